"""Multi-GPU message passing: spatial tiles + one-hop halo exchange of node latents.

The reference is single-process; this is new design for one
node of 8 MI355X.  The periodic box is cut into ``world`` spatial tiles, one per rank
(one process per GPU).  An edge belongs to its receiver's rank, so edge latents never
move; what a round needs from other ranks is the latent row ``x[src]`` of every
sender that lives elsewhere (a *ghost*).  Per round:

    pack owned rows peers asked for  ->  all-to-all-v over RCCL/xGMI  ->  ghost rows

``torch.distributed.all_to_all_single`` with split sizes is exactly the grouped
send/recv this needs: in a 2x2x2 periodic tiling every rank neighbours all 7 others,
one peer per xGMI link, so all links carry traffic at once and nothing is ring-bound.
The receive buffer *is* the ghost block of the local latent table (ghosts are stored
grouped by owner rank), so there is no unpack pass.

Index bookkeeping (ownership, ghost lists, global->local maps) is host logic done once
per graph with torch indexing; the per-round data path is HIP kernels + RCCL.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops, synthetic, training
from ._lib import CgnnError
from .graph_network import _next_projection, _node_half, _run_edge_stream, _run_round
from .training import NodeStreamSteps, _edge_rows  # noqa: F401  (_edge_rows: its tests reach it here)


# ----------------------------------------------------------------------------
# tiling
# ----------------------------------------------------------------------------

def tile_grid(world: int) -> Tuple[int, int, int]:
    """Near-cubic factorisation: 1->(1,1,1) 2->(2,1,1) 4->(2,2,1) 8->(2,2,2) ..."""
    dims = [1, 1, 1]
    n, p = world, 2
    factors = []
    while n > 1:
        while n % p == 0:
            factors.append(p)
            n //= p
        p += 1
    for f in sorted(factors, reverse=True):
        dims[dims.index(min(dims))] *= f
    return tuple(sorted(dims, reverse=True))


DECOMPOSITIONS = ("uniform", "balanced")
ROW_ORDERS = ("knn", "spatial")


@dataclass
class TilePlanes:
    """The cutting planes of a ``"balanced"`` decomposition (:func:`balanced_planes`) and their tile grid: ``x [px-1]``,
    ``y [px, py-1]`` (one row per x-slab), ``z [px, py, pz-1]`` (one row per (x, y) column), float32."""
    grid: Tuple[int, int, int]
    x: torch.Tensor
    y: torch.Tensor
    z: torch.Tensor

    def tensors(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.x, self.y, self.z


def _quantile_planes(v: torch.Tensor, p: int) -> torch.Tensor:
    """``c_j = s[(j * m) // p]``, ``j = 1 .. p-1``, ``s`` = ``v`` sorted ascending (``m`` = its length); zeros (no plane)
    for an empty segment.  ``-0`` counts as ``+0``."""
    m = v.numel()
    if m == 0 or p == 1:
        return torch.zeros(p - 1, dtype=torch.float32, device=v.device)
    s = torch.sort(v + 0.0).values
    return s[[(j * m) // p for j in range(1, p)]]


def _part_of(planes: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """``#{ j : c_j <= v }`` per element: ``planes [n, p-1]`` (each element's own planes) or ``[p-1]``."""
    return (planes <= v.unsqueeze(1)).sum(dim=1)


def balanced_planes(pos: torch.Tensor, box_size: float, world: int) -> TilePlanes:
    """Planes that cut the ``tile_grid(world)`` tiles at particle-count quantiles, nested x -> y -> z: for a segment of
    ``m`` particles and an axis with ``p`` parts the planes are ``c_j = s[(j * m) // p]`` (``s``: the segment's
    coordinates sorted ascending), and a coordinate ``v`` lies in part ``#{ j : c_j <= v }``.  All particles are cut
    into ``px`` slabs on x, every slab into ``py`` columns on y, every column into ``pz`` tiles on z.  A pure function
    of the position bits: every rank derives the same planes without communication.  Device tensors go through
    ``cgnn_balanced_planes`` (radix select); CPU tensors through this torch restatement (sort)."""
    del box_size        # the planes are data driven; the box only closes the end parts (tile_bounds)
    grid = px, py, pz = tile_grid(world)
    if pos.is_cuda:
        cx, cy, cz, _ = ops.balanced_planes(pos, grid)
        return TilePlanes(grid, cx, cy, cz)
    pos = pos.float()
    cx = _quantile_planes(pos[:, 0], px)
    ix = _part_of(cx, pos[:, 0])
    cy = torch.zeros((px, py - 1), dtype=torch.float32)
    cz = torch.zeros((px, py, pz - 1), dtype=torch.float32)
    for i in range(px):
        slab = torch.nonzero(ix == i).squeeze(1)
        cy[i] = _quantile_planes(pos[slab, 1], py)
        iy = _part_of(cy[i], pos[slab, 1])
        for j in range(py):
            cz[i, j] = _quantile_planes(pos[slab[iy == j], 2], pz)
    return TilePlanes(grid, cx, cy, cz)


def owner_of(pos: torch.Tensor, box_size: float, world: int, planes: Optional[TilePlanes] = None) -> torch.Tensor:
    """Rank owning each particle: the tile of the periodic box that contains it (equal-volume tiles, or the tiles of
    ``planes``)."""
    px, py, pz = tile_grid(world)
    if planes is not None:
        if tuple(planes.grid) != (px, py, pz):
            raise CgnnError(f"owner_of: planes of a {planes.grid} tile grid for a world of {world}")
        if pos.is_cuda:
            return ops.tile_classify(pos, planes.tensors(), want_counts=False)[0]
        ix = _part_of(planes.x, pos[:, 0])
        iy = _part_of(planes.y[ix], pos[:, 1])
        iz = _part_of(planes.z[ix, iy], pos[:, 2])
        return ((ix * py + iy) * pz + iz).to(torch.int32)
    g = torch.tensor([px, py, pz], device=pos.device, dtype=torch.float32)
    cell = torch.floor(pos / box_size * g).to(torch.int64)
    cell = torch.minimum(cell.clamp_min_(0), (g - 1).to(torch.int64))
    return ((cell[:, 0] * py + cell[:, 1]) * pz + cell[:, 2]).to(torch.int32)


# ----------------------------------------------------------------------------
# shard description
# ----------------------------------------------------------------------------

@dataclass
class Shard:
    rank: int
    world: int
    k: int
    n_owned: int
    n_ghost: int
    owned_global: torch.Tensor        # int64 [n_owned]  global ids, in the local (spatial) order
    ghost_global: torch.Tensor        # int64 [n_ghost]  grouped by owner rank
    src_local: torch.Tensor           # int32 [n_owned*k] rows of the local table [owned | ghosts]
    dst_local: torch.Tensor           # int32 [n_owned*k]
    edge_attr: torch.Tensor           # [n_owned*k, 4]
    recv_counts: List[int]            # ghost rows coming from each rank
    want_global: List[torch.Tensor] = field(default_factory=list)   # ids requested from each rank
    send_idx: Optional[torch.Tensor] = None    # int32 local owned rows to pack, grouped by destination
    send_counts: Optional[List[int]] = None
    x_feat: Optional[torch.Tensor] = None      # [n_owned, F] encoder inputs of the owned particles
    knn_ms: float = 0.0
    n_interior: int = 0               # owned rows [0, n_interior) have only owned senders (no halo needed)
    y_acc: Optional[torch.Tensor] = None       # [n_owned, 3] training targets of the owned particles
    y_temp_rate: Optional[torch.Tensor] = None  # [n_owned, 1]   (sharded_training_sample)

    @property
    def n_local(self) -> int:
        return self.n_owned + self.n_ghost


def tile_bounds(box_size: float, world: int, rank: int, planes: Optional[TilePlanes] = None):
    """``(lo [3], hi [3])`` of rank ``rank``'s tile (the inverse of :func:`owner_of`).  With ``planes``: part ``j`` of a
    segment spans ``[c_j, c_{j+1})``, ``c_0 = 0`` and ``c_p = box_size`` (reads the rank's planes back from the device)."""
    px, py, pz = tile_grid(world)
    ix, iy, iz = rank // (py * pz), (rank // pz) % py, rank % pz
    if planes is not None:
        if tuple(planes.grid) != (px, py, pz):
            raise CgnnError(f"tile_bounds: planes of a {planes.grid} tile grid for a world of {world}")
        cuts = torch.cat([planes.x, planes.y[ix], planes.z[ix, iy]]).tolist()       # one read-back
        lo, hi, off = [], [], 0
        for i, p in ((ix, px), (iy, py), (iz, pz)):
            c = [0.0] + cuts[off:off + p - 1] + [float(box_size)]
            lo.append(c[i])
            hi.append(c[i + 1])
            off += p - 1
        return lo, hi
    lo = [ix * box_size / px, iy * box_size / py, iz * box_size / pz]
    hi = [(ix + 1) * box_size / px, (iy + 1) * box_size / py, (iz + 1) * box_size / pz]
    return lo, hi


def _near_tile(pos: torch.Tensor, box_size: float, lo, hi, margin: float) -> torch.Tensor:
    """Particles within ``margin`` of the tile [lo, hi) along every axis, periodic (a superset of the margin ball)."""
    keep = torch.ones(pos.shape[0], dtype=torch.bool, device=pos.device)
    for a in range(3):
        width = hi[a] - lo[a]
        if width + 2 * margin >= box_size:
            continue                                  # the expanded tile covers this axis
        c = 0.5 * (lo[a] + hi[a])
        d = torch.abs(pos[:, a] - c)
        d = torch.minimum(d, box_size - d)            # periodic distance to the tile centre
        keep &= d <= 0.5 * width + margin
    return keep


def build_shard(pos_global: torch.Tensor, box_size: float, k: int, world: int, rank: int,
                knn_fn: Optional[Callable] = None, margin_factor: float = 2.0,
                decomposition: str = "uniform", *, row_order: str = "knn", min_image_edge_attr: bool = False,
                knn_grid: str = "uniform") -> Shard:
    """Everything rank ``rank`` can derive locally from the global positions: its owned set, their k-NN
    senders, the ghost set and the global->local renumbering.  ``knn_fn(pos, box, k, query_ids)`` defaults to
    the HIP k-NN; it returns ``(senders int32 [nq*k], edge_attr [nq*k, 4], order)``.

    The neighbour search runs over the rank's tile plus a margin, not over the whole box ("graph
    build"): margin = ``margin_factor`` x the radius that holds k particles at mean density.  It is then CHECKED --
    every owned particle's k-th neighbour must be closer than the margin, or some neighbour outside the subset could
    have been missed -- and doubled until the check holds (clustered inputs), so the result is the global one.

    ``decomposition``: ``"uniform"`` cuts tiles of equal volume; ``"balanced"`` cuts them at particle-count quantiles
    (:func:`balanced_planes`, kept as ``shard._planes``), so that every rank owns about ``N / world`` particles however
    clustered they are.  The tile is an axis-aligned box that holds every owned particle either way, so the search and
    its check are the same; only who owns a particle changes, never a result.

    ``knn_grid``: the cell grid of the default search (``ops.knn_periodic``'s ``grid``: ``"uniform"`` or ``"adaptive"``;
    same neighbours, ``"adaptive"`` is the faster one for a tile that holds a halo).  A caller's ``knn_fn`` is left
    alone.

    ``min_image_edge_attr``: the default search writes minimum-image edge features (``ops.knn_periodic``); the search
    over the tile's subset ranks the same periodic images as the global one, so the rows are the global graph's.  A
    caller's ``knn_fn`` decides for itself.

    ``row_order``: how the owned rows are numbered.  ``"knn"`` (default): the search's own cell order, which fills a
    cell through an atomic cursor, so two builds of one shard may number the particles of a cell differently (and
    float32 sums over the rows then differ in their last bits).  ``"spatial"``: ``training.spatial_order`` of the
    searched subset, a pure function of the positions: two builds give the same shard (``sharded_unrolled_loss``)."""
    if decomposition not in DECOMPOSITIONS:
        raise ValueError(f"build_shard: decomposition {decomposition!r}; known: {DECOMPOSITIONS}")
    if row_order not in ROW_ORDERS:
        raise ValueError(f"build_shard: row_order {row_order!r}; known: {ROW_ORDERS}")
    ops.check_knn_grid(knn_grid, "build_shard")
    ops.check_min_image(min_image_edge_attr, "build_shard")
    dev = pos_global.device
    n_total = pos_global.shape[0]
    planes = balanced_planes(pos_global, box_size, world) if decomposition == "balanced" else None
    classify = planes is not None and dev.type == "cuda"       # owner, counts and the margin mask in one HIP pass
    counts = None
    if not classify:
        owner = owner_of(pos_global, box_size, world, planes)
    knn = knn_fn or (lambda p, b, kk, q: ops.knn_periodic(p, b, kk, query_ids=q, want_edge_attr=True,
                                                          want_order=True, grid=knn_grid,
                                                          min_image_edge_attr=min_image_edge_attr))
    t0 = time.perf_counter()
    search_ms = 0.0

    def timed_knn(p, b, kk, q):     # device time of the neighbour search alone (the torch glue around it is host-bound)
        nonlocal search_ms
        if dev.type != "cuda":
            return knn(p, b, kk, q)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = knn(p, b, kk, q)
        e1.record()
        e1.synchronize()
        search_ms += e0.elapsed_time(e1)
        return out

    lo, hi = tile_bounds(box_size, world, rank, planes)
    margin = margin_factor * box_size * (3.0 * k / (4.0 * 3.141592653589793 * max(n_total, 1))) ** (1.0 / 3.0)
    searches = 0
    while True:
        searches += 1
        if classify:        # near = within the margin of the tile, or owned (as below), from cgnn_tile_classify
            first = counts is None
            own_, counts_, near = ops.tile_classify(pos_global, planes.tensors(), rank, lo, hi, margin, box_size,
                                                    want_owner=first, want_counts=first)
            if first:
                owner, counts = own_, counts_
            if world == 1:
                near = None
        else:
            near = _near_tile(pos_global, box_size, lo, hi, margin) if world > 1 else None
            if near is not None:
                near |= owner == rank      # owner_of clamps coordinates outside [0, box) into edge tiles: owned is always searched
        whole = near is None or bool(near.all())
        sub = None if whole else torch.nonzero(near).squeeze(1)        # ascending global ids: ties order as globally
        pos_sub = pos_global if whole else pos_global[sub].contiguous()
        own_sub = owner if whole else owner[sub]
        owned_s = torch.nonzero(own_sub == rank).squeeze(1)            # indices into the subset
        # a one-query pass builds the cell grid and yields the spatial (cell-sorted) order, so that the local
        # numbering is cache friendly; then the real pass over the owned queries in that order
        if owned_s.numel() and row_order == "spatial":
            order = training.spatial_order(pos_sub, box_size).long()
            owned_s = order[own_sub[order] == rank]
        elif owned_s.numel():
            _, _, order = timed_knn(pos_sub, box_size, k, owned_s[:1].to(torch.int32))
            if order is not None:
                order = order.long()
                owned_s = order[own_sub[order] == rank]
        if owned_s.numel():
            senders_s, edge_attr, _ = timed_knn(pos_sub, box_size, k, owned_s.to(torch.int32))
        else:           # an empty tile (balanced tiles of coincident coordinates): no query, nothing to search
            senders_s = torch.empty(0, dtype=torch.int32, device=dev)
            edge_attr = torch.empty((0, 4), dtype=torch.float32, device=dev)
        if whole or owned_s.numel() == 0:
            break
        # k-th neighbour distance (minimum image) of every owned particle against the margin
        kth = senders_s.view(-1, k)[:, k - 1].long()
        dlt = torch.abs(pos_sub[kth] - pos_sub[owned_s])
        dlt = torch.minimum(dlt, box_size - dlt)
        if float(dlt.norm(dim=1).max()) <= margin:
            break
        margin *= 2.0
    owned = owned_s if whole else sub[owned_s]
    senders = senders_s.long() if whole else sub[senders_s.long()]
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    build_ms = (time.perf_counter() - t0) * 1e3          # selection of the tile + margin subset, both searches, the check
    knn_ms = search_ms if dev.type == "cuda" else build_ms
    n_owned = owned.numel()
    senders = senders.long()
    remote = owner[senders] != rank
    # interior receivers (every sender owned) first, boundary receivers last, spatial order kept inside each group:
    # a round's interior half can then run while the halo exchange is still in flight
    is_boundary = remote.view(n_owned, k).any(dim=1) if n_owned else remote.new_zeros((0,))
    n_interior = int((~is_boundary).sum())
    if 0 < n_interior < n_owned:
        regroup = torch.cat([torch.nonzero(~is_boundary).squeeze(1), torch.nonzero(is_boundary).squeeze(1)])
        owned = owned[regroup]
        senders = senders.view(n_owned, k)[regroup].reshape(-1)
        edge_attr = edge_attr.view(n_owned, k, -1)[regroup].reshape(n_owned * k, -1).contiguous()
        remote = remote.view(n_owned, k)[regroup].reshape(-1)
    ghosts = torch.unique(senders[remote])
    g_owner = owner[ghosts].long()
    perm = torch.argsort(g_owner * n_total + ghosts)      # group by owner rank, ascending id inside
    ghosts = ghosts[perm]
    g_owner = g_owner[perm]
    recv_counts = torch.bincount(g_owner, minlength=world).tolist()
    g2l = torch.full((n_total,), -1, dtype=torch.int32, device=dev)
    g2l[owned] = torch.arange(n_owned, dtype=torch.int32, device=dev)
    g2l[ghosts] = n_owned + torch.arange(ghosts.numel(), dtype=torch.int32, device=dev)
    src_local = g2l[senders].contiguous()
    dst_local = torch.arange(n_owned, dtype=torch.int32, device=dev).repeat_interleave(k)
    want = list(torch.split(ghosts, recv_counts))
    sh = Shard(rank, world, k, n_owned, ghosts.numel(), owned, ghosts, src_local, dst_local, edge_attr,
               recv_counts, want_global=want, knn_ms=knn_ms, n_interior=n_interior)
    sh._g2l = g2l
    sh._owner = owner            # every particle's rank (the sharded rollout sizes its send blocks from it)
    sh._planes = planes          # the balanced decomposition's cutting planes (None: equal-volume tiles)
    sh._counts = counts          # int64 [world] on the device (cgnn_tile_classify), or None: bincount of _owner
    sh.subset_build_ms = build_ms
    sh.searches = searches       # 1: the first margin held; every further one doubled it
    sh.subset_rows = pos_sub.shape[0]
    return sh


def finish_shard(sh: Shard, requests_from_peers: Sequence[torch.Tensor]) -> Shard:
    """``requests_from_peers[r]`` = global ids rank r wants from us -> local rows to pack, grouped by r."""
    idx = [sh._g2l[req.long()] for req in requests_from_peers]
    for r, t in enumerate(idx):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= sh.n_owned):
            raise RuntimeError(f"rank {sh.rank}: rank {r} requested rows this rank does not own")
    sh.send_counts = [int(t.numel()) for t in idx]
    sh.send_idx = torch.cat(idx).to(torch.int32).contiguous() if idx else torch.empty(0, dtype=torch.int32)
    return sh


def _comm_device(tensor_device: torch.device, group=None) -> torch.device:
    """Device the process group moves data on: the tensors' own device with RCCL ("nccl"); the host with gloo
    (CPU tests, and the single-GPU rehearsal of the multi-rank path, which stages through host memory)."""
    import torch.distributed as dist
    return tensor_device if dist.get_backend(group) == "nccl" else torch.device("cpu")


def _collective(collective: Callable, out: torch.Tensor, *inputs: torch.Tensor, group=None,
                **kwargs) -> Callable[[], torch.Tensor]:
    """``collective(out, *inputs, group=group, **kwargs)``, a ``torch.distributed`` collective, run on the group's device
    (:func:`_comm_device`); device tensors are staged through host memory under gloo.  No ``inputs``: ``out`` is
    reduced in place.  Returns ``wait()``, which waits for the collective (RCCL, ``async_op=True``: the current stream
    waits) and returns ``out``, holding the result."""
    cdev = _comm_device(out.device, group)
    if cdev == out.device:
        host = out
    else:
        host = torch.empty(out.shape, dtype=out.dtype, device=cdev) if inputs else out.to(cdev)
    work = collective(host, *[t.to(cdev) for t in inputs], group=group, **kwargs)

    def wait() -> torch.Tensor:
        if work is not None:
            work.wait()
        return out if host is out else out.copy_(host)
    return wait


def exchange_requests(sh: Shard, group=None, finish: Optional[Callable] = None) -> Shard:
    """Setup-time all-to-all of the ghost id lists (sizes, then ids).  ``finish(sh, requests)`` makes the send plan
    (:func:`finish_shard`; :func:`finish_shard_by_search` for a shard numbered in subset space)."""
    import torch.distributed as dist
    counts_out = torch.tensor(sh.recv_counts, dtype=torch.int64, device=sh.owned_global.device)
    counts_in = _collective(dist.all_to_all_single, torch.empty_like(counts_out), counts_out, group=group)().tolist()
    recv = torch.empty(int(sum(counts_in)), dtype=torch.int64, device=counts_out.device)
    _collective(dist.all_to_all_single, recv, sh.ghost_global.contiguous(), output_split_sizes=counts_in,
                input_split_sizes=sh.recv_counts, group=group)()
    return (finish or finish_shard)(sh, list(torch.split(recv, counts_in)))


def sharded_training_sample(position_seq: torch.Tensor, temperature_seq: torch.Tensor, metadata: dict,
                            target_position: torch.Tensor, target_temperature: torch.Tensor, noise_std: float,
                            num_neighbors: int, dt: float, box_size: float, world: int, rank: int, noise_seed: int,
                            noise_draw: int = 0, device=None, decomposition: str = "uniform", *,
                            min_image_edge_attr: bool = False, knn_grid: str = "uniform") -> Shard:
    """Rank ``rank``'s part of the training sample ``data_utils.preprocess(..., noise_rng="device")`` makes on one GPU,
    with the same bits: the window ``[W, N, 3]`` / ``[W, N(, 1)]`` and the next frame ``[N, 3]`` / ``[N(, 1)]`` (or
    ``[1, N, ...]``) of ALL particles go in, every rank passing the same data, ``noise_seed`` and ``noise_draw``.

    The device noise is a function of (seed, draw, particle id, step), so every rank first makes the noisy wrapped last
    frame of all N particles (identical bits everywhere: ``owner_of`` agrees without communication) and builds its
    shard on it, then makes ``x``, ``y_acc`` and ``y_temp_rate`` for the rows it owns only.  Returns the shard as
    :func:`build_shard` does, with ``x_feat``, ``y_acc [n_owned, 3]`` and ``y_temp_rate [n_owned, 1]`` set (local row
    order, ``owned_global``); :func:`exchange_requests` / :func:`finish_shard` remain the caller's next call.
    ``decomposition``: as in :func:`build_shard` (the planes of ``"balanced"`` come from the noisy frame, the same on
    every rank); ``knn_grid``, ``min_image_edge_attr``: as there."""
    ops.check_knn_grid(knn_grid, "sharded_training_sample")
    ops.check_min_image(min_image_edge_attr, "sharded_training_sample")
    if device is None:
        if not position_seq.is_cuda:
            raise CgnnError("sharded_training_sample: pass device= or device-resident windows")
        device = position_seq.device
    device = torch.device(device)
    dt, box_size = float(dt), float(box_size)
    n = position_seq.shape[1]
    pos_w = position_seq.to(device).float().contiguous()
    tmp_w = temperature_seq.to(device).float().contiguous()
    if target_position.numel() != n * 3 or target_temperature.numel() != n:
        raise CgnnError(f"sharded_training_sample: targets {tuple(target_position.shape)} / "
                        f"{tuple(target_temperature.shape)} do not hold [N, 3] / [N] for N = {n}")
    tgt_p = target_position.to(device).float().reshape(n, 3)
    tgt_t = target_temperature.to(device).float().reshape(n)
    stats = ops.integration_stats(metadata)
    recent = ops.training_sample(pos_w, tmp_w, metadata, dt, box_size, noise_std, noise_seed, noise_draw,
                                 want=("recent_pos",), stats=stats)["recent_pos"]
    sh = build_shard(recent, box_size, int(num_neighbors), world, rank, decomposition=decomposition,
                     knn_grid=knn_grid, min_image_edge_attr=min_image_edge_attr)
    own = ops.training_sample(pos_w, tmp_w, metadata, dt, box_size, noise_std, noise_seed, noise_draw, tgt_p, tgt_t,
                              rows=sh.owned_global, want=("x", "y_acc", "y_temp_rate"), stats=stats)
    sh.x_feat, sh.y_acc, sh.y_temp_rate = own["x"], own["y_acc"], own["y_temp_rate"].reshape(-1, 1)
    return sh


# ----------------------------------------------------------------------------
# halo exchange (per round)
# ----------------------------------------------------------------------------

class HaloExchange:
    """Fills the ghost block ``table[n_owned:]`` from the owners' rows ``table[:n_owned]``."""

    def __init__(self, sh: Shard, group=None, pack_fn: Optional[Callable] = None):
        self.sh, self.group = sh, group
        self.pack = pack_fn or (lambda table, idx, out: ops.gather_rows(table, idx, out))
        self._buf = None
        self._ret = None

    def start(self, table: torch.Tensor):
        """Pack the rows the peers asked for and start the all-to-all into ``table``'s ghost block; returns a handle
        for :meth:`finish`.  Kernels enqueued in between run under the exchange (they must not touch ghost rows)."""
        import torch.distributed as dist
        sh = self.sh
        width = table.shape[1]
        if self._buf is None or self._buf.shape != (sh.send_idx.numel(), width) or self._buf.device != table.device:
            self._buf = torch.empty((sh.send_idx.numel(), width), dtype=table.dtype, device=table.device)
        if sh.send_idx.numel():
            self.pack(table, sh.send_idx, self._buf)
        return _collective(dist.all_to_all_single, table[sh.n_owned:], self._buf, output_split_sizes=sh.recv_counts,
                           input_split_sizes=sh.send_counts, group=self.group, async_op=True)

    def finish(self, handle) -> None:
        handle()                          # RCCL: the current stream waits for the exchange

    def __call__(self, table: torch.Tensor) -> None:
        self.finish(self.start(table))

    # backward: the reverse all-to-all (the forward's split sizes swapped)
    def start_return(self, grad_ghost: torch.Tensor):
        """Send the gradient of every ghost row (``grad_ghost`` [n_ghost, W], grouped by owner like the ghost block) back
        to its owner; returns a handle for :meth:`finish_return`.  What comes back is, per peer in rank order, the
        gradients of the rows this rank sent it (``send_idx`` order): [sum(send_counts), W]."""
        import torch.distributed as dist
        sh = self.sh
        shape = (int(sum(sh.send_counts)), grad_ghost.shape[1])
        if self._ret is None or tuple(self._ret.shape) != shape or self._ret.device != grad_ghost.device:
            self._ret = torch.empty(shape, dtype=grad_ghost.dtype, device=grad_ghost.device)
        return _collective(dist.all_to_all_single, self._ret, grad_ghost, output_split_sizes=sh.send_counts,
                           input_split_sizes=sh.recv_counts, group=self.group, async_op=True)

    def finish_return(self, handle) -> torch.Tensor:
        """Wait for :meth:`start_return`; returns the received gradient rows on the gradients' device."""
        return handle()


def halo_return_plan(send_idx: torch.Tensor, send_counts: Sequence[int], n_owned: int):
    """The plan of ``ops.halo_return_add`` for one shard: ``(rows, seg_ptr, col)`` int32 on ``send_idx``'s device.
    Position p of the reverse exchange's output carries the gradient for owned row ``send_idx[p]`` (the forward's pack
    order: grouped by peer, ascending rank).  ``rows``: the distinct requested rows, ascending; ``col[seg_ptr[j] ..
    seg_ptr[j + 1]]``: row j's positions, ascending, hence in ascending peer rank.  Validated here, once per shard."""
    idx = send_idx.reshape(-1).long()
    counts = [int(c) for c in send_counts]
    if any(c < 0 for c in counts) or sum(counts) != idx.numel():
        raise CgnnError(f"halo_return_plan: send counts {counts} do not add up to the {idx.numel()} rows of send_idx")
    if idx.numel() >= 2 ** 31:
        raise CgnnError("halo_return_plan: more than 2^31 - 1 returned rows")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_owned):
        raise CgnnError(f"halo_return_plan: send_idx holds rows outside the {n_owned} owned rows")
    vals, pos = torch.sort(idx, stable=True)
    rows, cnt = torch.unique_consecutive(vals, return_counts=True)
    seg_ptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(cnt, 0, out=seg_ptr[1:])
    return rows.to(torch.int32), seg_ptr.to(torch.int32), pos.to(torch.int32)


# ----------------------------------------------------------------------------
# sharded forward
# ----------------------------------------------------------------------------

def _src_part(runner, a: int, b: int) -> torch.Tensor:
    """The sender list of ``runner``'s owned receivers [a, b) as one tensor OBJECT per part (the aggregation plan is
    cached on it)."""
    parts = runner.__dict__.setdefault("_src_parts", {})
    if (a, b) not in parts:
        k = runner.sh.k
        parts[(a, b)] = runner.sh.src_local[a * k:b * k]
    return parts[(a, b)]


def _exchange_rounds(halo, n_rounds: int, table_of: Callable, nodes: Callable, overlap: bool) -> None:
    """The rounds of a shard runner: round ``i``'s table ``table_of(i)`` gets its ghost rows from ``halo``, and
    ``nodes(i, part)`` runs the round for the owned receivers of ``part``.  With ``overlap`` the exchange runs under
    the ``"interior"`` receivers (no ghost sender) and the ``"boundary"`` ones follow it; else ``"all"`` run after it."""
    for i in range(n_rounds):
        table = table_of(i)
        if overlap:
            handle = halo.start(table)
            nodes(i, "interior")
            halo.finish(handle)
            nodes(i, "boundary")
        else:
            halo(table) if callable(halo) else halo.finish(halo.start(table))
            nodes(i, "all")


class ShardedForward:
    """``EncodeProcessDecode.forward`` over one spatial tile.  ``halo(table)`` must fill the ghost rows of
    ``table`` ([n_owned + n_ghost, D]) from their owners; by default it is the RCCL all-to-all above.
    Returns the predictions of the owned particles (local order; ``shard.owned_global`` maps them back).

    A rank that owns nothing (a balanced tile between coincident planes) has no receivers, hence no edges and no
    ghosts: it launches nothing, takes part in every exchange with empty blocks and returns empty predictions."""

    def __init__(self, model, shard: Shard, halo: Optional[Callable] = None):
        self.model, self.sh = model, shard
        self.halo = halo if halo is not None else HaloExchange(shard)
        self._bufs = None

    def _buffers(self, D: int, H: int, dev):
        sh = self.sh
        key = (D, H, dev, self.model.edge_precision, self.fused, self.plan.p_format)
        if self._bufs is None or self._bufs[0] != key:
            x_all = torch.empty((sh.n_local, D), dtype=torch.float32, device=dev)
            pdt = ops.p_format_dtype(self.plan.p_format)
            if self.fused:      # every round's tables are kept for the one-launch edge stream (same row stride for both)
                L = len(self.P["rounds"])
                ps = torch.empty((L, sh.n_local, H), dtype=pdt, device=dev)
                pd = torch.empty((L, sh.n_local, H), dtype=pdt, device=dev)
            else:
                ps = torch.empty((sh.n_local, H), dtype=pdt, device=dev)
                pd = torch.empty((sh.n_owned, H), dtype=pdt, device=dev)
            agg = torch.empty((sh.n_owned, D), dtype=torch.float32, device=dev)
            # fused mode updates the node latents out of place (interior rows are rewritten while boundary receivers
            # still gather the old ones): a second table, swapped every round
            x_alt = torch.empty_like(x_all) if self.fused else None
            self._bufs = (key, x_all, ps, pd, agg, x_alt)
        return self._bufs[1:]

    # the pieces are separate methods so that a single-process test can interleave several shards
    def encode(self):
        m, sh = self.model, self.sh
        P = self.P = m._pack(sh.x_feat.shape[1], sh.edge_attr.shape[1])
        D = m._latent_size
        self.empty = sh.n_owned == 0
        if self.empty:
            self.fused, self._edges_pending, self.el = False, False, None
            self.x_all = torch.empty((0, D), dtype=torch.float32, device=sh.x_feat.device)
            return
        H = P["rounds"][0].ws.out_dim if P["rounds"] else D
        # the same plan as on one GPU: under the reference data flow (x_j) the node stream runs round by round with its
        # halo exchanges and leaves every round's Ps / Pd behind; the edge stream then is one launch
        self.plan = m._stream_plan(P, sh.k, sh.src_local.numel(), sh.edge_attr)
        self.fused = self.plan.fused
        self.x_all, self.ps, self.pd, self.agg, self.x_alt = self._buffers(D, H, sh.x_feat.device)
        ops.mlp_rows(P["enc_node"], sh.x_feat, out=self.x_all[:sh.n_owned])
        self._projected = False
        self._edges_pending = False
        self.el = None if self.plan.enc_in_stream else ops.mlp_rows(P["enc_edge"], sh.edge_attr, tiled=True)
        self.e_upd = self.el.empty_like() if m.message_source == "edge" else None

    def round(self, i: int):
        if self.empty:
            return
        if self.fused:
            return self._round_nodes(i)
        sh, rounds = self.sh, self.P["rounds"]
        p = rounds[i]
        # sender projections of the ghost rows that just arrived (receivers are always owned: no Pd for ghosts)
        if sh.n_ghost:
            ops.project_nodes(p.ws, None, self.x_all[sh.n_owned:], self.ps[sh.n_owned:], None, p.p_format)
        nxt = rounds[i + 1] if i + 1 < len(rounds) else None
        _, self.el, self._projected = _run_round(
            p, self.x_all, self.el, sh.src_local, sh.dst_local, sh.k, self.model.message_source, True,
            x_out=self.x_all[:sh.n_owned], e_out=self.el, scratch=(self.ps, self.pd, self.agg, self.e_upd),
            projected=self._projected, next_round=nxt, n_recv=sh.n_owned)

    def _interior_launch_rows(self) -> int:
        """Rows of the "interior" launches: ``n_interior`` rounded DOWN to whole grid waves of the node kernel.  A launch of
        s 128-row steps on c workgroups (one per CU) takes ceil(s / c) step times, so the remainder of the interior rows cost
        a whole extra step time there -- 849 steps on 256 CUs: four step times for 3.3 of work at 125 k rows per rank -- and
        nothing in the boundary launch, which is far from full; rows that need no ghost may run after the exchange just as well."""
        ni = self.sh.n_interior
        cached = self.__dict__.get("_ni_launch")
        if cached is not None and cached[0] == ni:
            return cached[1]
        dev = self.sh.x_feat.device
        rows = ni
        if dev.type == "cuda":
            wave_rows = 128 * torch.cuda.get_device_properties(dev).multi_processor_count
            if ni >= wave_rows:
                rows = ni - ni % wave_rows
        self._ni_launch = (ni, rows)
        return rows

    def _round_nodes(self, i: int, part: str = "all"):
        """Fused mode: the node half of round ``i`` for the owned rows of ``part``: ``"interior"`` (receivers whose
        senders are all owned: needs no ghost row, runs under the halo exchange), ``"boundary"`` (the rest, after the
        exchange; also projects the ghost rows) or ``"all"``.  Reads ``x_all``, writes ``x_alt``; the tables swap
        when the round is complete."""
        if self.empty:
            return
        sh = self.sh
        rounds = self.P["rounds"]
        p, fmt = rounds[i], self.plan.p_format
        no, ni = sh.n_owned, self._interior_launch_rows()
        a, b = {"all": (0, no), "interior": (0, ni), "boundary": (ni, no)}[part]
        if part != "interior" and sh.n_ghost:
            ops.project_nodes(p.ws, None, self.x_all[no:], self.ps[i][no:], None, fmt)
        if b > a:
            if i == 0:
                ops.project_nodes(p.ws, p.wd, self.x_all[a:b], self.ps[0][a:b], self.pd[0][a:b], fmt)
            nxt = _next_projection(p, rounds[i + 1], self.ps[i + 1], self.pd[i + 1], fmt) if i + 1 < len(rounds) else None
            _node_half((p.node, p.wx, p.wa), self.x_all, _src_part(self, a, b), None, sh.k, a, b, self.agg, self.x_alt, nxt)
        if part != "interior":
            self.x_all, self.x_alt = self.x_alt, self.x_all
            self._edges_pending = i + 1 == len(rounds)

    def finish_edges(self):
        """Fused mode: all edge updates in one launch, once the last round's node half has run."""
        if self.fused and self._edges_pending:
            sh = self.sh
            self.el = _run_edge_stream(self.P, self.plan, self.ps, self.pd, sh.src_local, sh.dst_local, self.el,
                                       sh.edge_attr, sh.k)
            self._edges_pending = False

    def decode(self) -> dict:
        self.finish_edges()
        if self.empty:
            dev = self.x_all.device
            return {"acceleration": torch.empty((0, self.P["dec_acc"].out_dim), dtype=torch.float32, device=dev),
                    "temp_rate": torch.empty((0, 1), dtype=torch.float32, device=dev)}
        x_own = self.x_all[:self.sh.n_owned]
        return {"acceleration": ops.mlp_rows(self.P["dec_acc"], x_own),
                "temp_rate": ops.mlp_rows(self.P["dec_tr"], x_own)}

    def __call__(self) -> dict:
        with torch.no_grad():
            self.encode()
            # x_j aggregation and the sender projections both read ghost latents of the current round
            overlap = self.fused and hasattr(self.halo, "start") and 0 < self.sh.n_interior
            _exchange_rounds(self.halo, len(self.P["rounds"]), lambda i: self.x_all,
                             lambda i, part: self._round_nodes(i, part) if self.fused else self.round(i), overlap)
            return self.decode()


# ----------------------------------------------------------------------------
# sharded training (message_source="x_j")
# ----------------------------------------------------------------------------

def _group_up() -> bool:
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def _all_reduce_(t: torch.Tensor, group=None) -> torch.Tensor:
    """In-place SUM over the group (no process group up: a world of one, ``t`` as it is)."""
    import torch.distributed as dist
    if not _group_up():
        return t
    return _collective(dist.all_reduce, t, group=group)()


class _AllReduceSum(torch.autograd.Function):
    """Sum over the ranks of a value every rank then uses in full; the backward is the identity (each rank's
    contribution enters the sum with weight one, and the term built on it is replicated, not summed)."""

    @staticmethod
    def forward(ctx, t, group):
        return _all_reduce_(t.detach().clone(), group)

    @staticmethod
    def backward(ctx, g):
        return g, None


def sharded_training_loss(pred: dict, y_acc: torch.Tensor, y_tr: torch.Tensor, n_total: int, dt: float,
                          acc_w: float = 1.0, tr_w: float = 1.0, mom_w: float = 0.0, group=None, batch=None,
                          terms: bool = False):
    """The reference's ``combined_loss`` (train.py:255-260) of a snapshot split over the ranks, from this rank's owned
    predictions ``pred`` and targets.  Returns ``(loss_to_backprop, global_value)``:

    * the MSE terms are this rank's sums of squares over the *global* element counts, so that the ranks' terms add up
      to the global means;
    * the momentum term is built on the global per-graph column sums (``ops.segment_colsum`` in float64, summed over
      the ranks with an identity backward): it is the same on every rank, and each rank's rows receive their share
      of its gradient once;
    * ``global_value`` (0-d float64) is the all-reduced loss, the value ``combined_loss`` has on the whole snapshot.

    Summing the ranks' parameter gradients of ``loss_to_backprop`` gives the gradient of ``global_value``.

    ``terms=True`` returns ``(loss_to_backprop, global_value, global_terms)``, ``global_terms`` float64 ``[3]``: the two
    global means and the momentum term, what ``unrolled_loss`` reports per step (the same collectives: the two partial
    sums travel in one all-reduce)."""
    from .losses import _SegmentColsum
    if batch is not None:
        raise NotImplementedError("sharded training takes one graph (snapshot) per shard; multi-graph batches are not "
                                  "supported")
    acc, tr = pred["acceleration"], pred["temp_rate"]
    acc_part = ((acc - y_acc) ** 2).sum() / float(n_total * acc.shape[1])
    tr_part = ((tr - y_tr) ** 2).sum() / float(n_total * tr.shape[1])
    mse = acc_w * acc_part + tr_w * tr_part
    sums = _AllReduceSum.apply(_SegmentColsum.apply(acc, None, 1), group)          # [1, 3] float64, global
    mom = (mom_w * torch.sum((sums * float(dt)) ** 2)).to(torch.float32)
    if terms:
        parts = _all_reduce_(torch.stack([acc_part.detach().double(), tr_part.detach().double()]), group)
        value = acc_w * parts[0] + tr_w * parts[1] + mom.detach().double()
        return mse + mom, value, torch.stack([parts[0], parts[1], mom.detach().double()])
    part = mse.detach().double().reshape(1).clone()
    value = _all_reduce_(part, group)[0] + mom.detach().double()
    return mse + mom, value


def _all_reduce_grads(grads: Sequence[torch.Tensor], group=None) -> List[torch.Tensor]:
    """The ranks' parameter gradients summed by ONE all-reduce of a flat buffer; -> views of it shaped like ``grads``."""
    flat = torch.cat([g.reshape(-1) for g in grads])
    _all_reduce_(flat, group)
    out, off = [], 0
    for g in grads:
        out.append(flat[off:off + g.numel()].view_as(g))
        off += g.numel()
    return out


class ShardedTraining(NodeStreamSteps):
    """A training step of ``EncodeProcessDecode`` (``message_source="x_j"``, ``train_precision`` "fp32" / "fp32x3") over one
    spatial tile.  An edge model with ``model.train_edge_messages`` gets a :class:`ShardedEdgeTraining` instead (the
    constructor picks it).  Under x_j: the node stream of :class:`training._NodeStream` on the owned rows, with one halo exchange of the f32
    latents per round in the forward and one reverse exchange of their gradients per round in the backward.

    Forward of round i: ``x_i`` (owned rows) is staged into the local table ``[owned | ghosts]``, the exchange fills the
    ghosts while the interior receivers (no ghost sender) aggregate and run the node block, then the boundary receivers
    do.  Only the owned rows of ``x_i`` and ``agg_i`` are kept for the backward.

    Backward of round i (``dx`` = dL/dx_{i+1} on the owned rows): ``du1, du2 = backward of the node MLP``; the ghost pass
    ``A^T du2`` on the ghost rows of the local sender CSR, written into the send buffer; the reverse all-to-all starts;
    the owned pass ``dx <- dx + du1 + A^T du2`` runs under it; the returned rows are added into ``dx``
    (``ops.halo_return_add``).  The encoder's backward gives ``dx0`` of the owned particles.  The ranks' parameter
    gradients are summed by ONE all-reduce of a flat buffer, so ``.grad`` is the global gradient on every rank.

    The pieces are methods so that one process can interleave several shards (tests); ``__call__`` runs them through a
    ``torch.autograd.Function`` for a real process group.  ``halo`` needs ``start`` / ``finish`` and ``start_return`` /
    ``finish_return`` (:class:`HaloExchange`, the default).

    A rank that owns nothing (``n_owned == 0``, hence no edges and no ghosts) launches no kernel: every piece returns
    empty rows or zero parameter gradients, and the exchanges and the gradient all-reduce around the pieces run as on
    every other rank, with empty blocks."""

    def __new__(cls, model, shard: Shard, halo=None, group=None):
        if cls is ShardedTraining and model.message_source == "edge" and getattr(model, "train_edge_messages", False):
            cls = ShardedEdgeTraining
        return super().__new__(cls)

    def __init__(self, model, shard: Shard, halo=None, group=None):
        edge = isinstance(self, ShardedEdgeTraining)
        if model.message_source != ("edge" if edge else "x_j") or (edge and not getattr(model, "train_edge_messages", False)):
            raise NotImplementedError("sharded training is built for message_source='x_j', and for 'edge' with "
                                      "model.train_edge_messages = True")
        if getattr(model, "train_edge_stream", False):
            raise NotImplementedError("sharded training does not run the (dead) edge stream: model.train_edge_stream "
                                      "is single-GPU only")
        if getattr(shard, "batch", None) is not None:
            raise NotImplementedError("sharded training takes one graph (snapshot) per shard; multi-graph batches are "
                                      "not supported")
        if shard.send_idx is None:
            raise CgnnError("ShardedTraining: the shard has no send plan (finish_shard / exchange_requests first)")
        self.model, self.sh, self.group = model, shard, group
        self.halo = halo if halo is not None else HaloExchange(shard, group)
        self.packs = None
        self._table = None
        self._ghost = None
        self._csr = None
        self._plan = None

    # -- set-up ------------------------------------------------------------------------------------------------------
    def _prepare(self, x0: torch.Tensor) -> None:
        m, sh = self.model, self.sh
        with torch.no_grad():
            m._materialize_all(x0.shape[1], sh.edge_attr.shape[1])
            self.packs = m._train_packs()       # refuses what the training kernels do not take (CgnnError)
        if self._csr is None and sh.n_owned:
            self._csr = ops.SenderCsr(sh.src_local, sh.dst_local, sh.n_local)       # senders <- receivers, once per shard
            self._plan = halo_return_plan(sh.send_idx.to(x0.device), sh.send_counts, sh.n_owned)

    # -- forward pieces ----------------------------------------------------------------------------------------------
    def encode(self, x0: Optional[torch.Tensor] = None) -> None:
        """Node encoder on the owned rows (``x0`` defaults to ``shard.x_feat``)."""
        sh = self.sh
        x0 = (sh.x_feat if x0 is None else x0).detach().float().contiguous()
        if x0.shape[0] != sh.n_owned:
            raise CgnnError(f"ShardedTraining: {x0.shape[0]} input rows for {sh.n_owned} owned particles")
        self._prepare(x0)
        D = self.packs.latent
        if sh.n_owned == 0:
            self.x0, self.xs, self.aggs = x0, [x0.new_empty((0, D))], []
        else:
            self._encode(self.packs, x0)
        if self._table is None or tuple(self._table.shape) != (sh.n_local, D) or self._table.device != x0.device:
            self._table = torch.empty((sh.n_local, D), dtype=torch.float32, device=x0.device)

    def stage(self, i: int) -> torch.Tensor:
        """Round ``i``'s local table: the owned rows hold ``x_i``; the exchange is to fill the ghost rows."""
        self._table[:self.sh.n_owned].copy_(self.xs[i])
        self._new_round()
        return self._table

    def round_nodes(self, i: int, part: str = "all") -> None:
        """Aggregation and node block of round ``i`` for the owned receivers of ``part``: ``"interior"`` (no ghost sender:
        may run under the exchange), ``"boundary"`` (after it) or ``"all"``."""
        sh = self.sh
        no, ni = sh.n_owned, sh.n_interior
        a, b = {"all": (0, no), "interior": (0, ni), "boundary": (ni, no)}[part]
        if b > a:
            self._round_nodes(i, self._table, _src_part(self, a, b), None, sh.k, a, b)

    def decode(self):
        if self.sh.n_owned == 0:
            p, x = self.packs, self.x0
            return x.new_empty((0, p.dec_acc.out_dim)), x.new_empty((0, p.dec_tr.out_dim))
        return super().decode()

    # -- backward pieces (local_grads: NodeStreamSteps) ------------------------------------------------------------------
    def _zero_grads(self, packed) -> None:
        """No rows: the parameter gradients of the MLPs ``packed`` are zeros (this rank's term of the all-reduce)."""
        for m in packed:
            self.grads_of[id(m)] = [torch.zeros_like(q, memory_format=torch.contiguous_format) for q in m.params()]

    def decode_backward(self, d_acc: Optional[torch.Tensor], d_tr: Optional[torch.Tensor]) -> None:
        if self.sh.n_owned == 0:
            self.grads_of, self.scratch = {}, None
            self._zero_grads(self.packs.all)
            self.dx = self.x0.new_empty((0, self.packs.latent))
            return
        super().decode_backward(d_acc, d_tr)

    def encode_backward(self, need_dx0: bool = True, **more) -> Optional[torch.Tensor]:
        if self.sh.n_owned == 0:
            self.dx = None
            return torch.zeros_like(self.x0) if need_dx0 else None
        return super().encode_backward(need_dx0, **more)

    def round_backward_local(self, i: int) -> torch.Tensor:
        """Steps 1-2 of round ``i``: the node MLP's backward on the owned rows, then ``A^T du2`` for the ghost rows,
        written into (and returned as) the send buffer of the reverse exchange, [n_ghost, D]."""
        sh = self.sh
        if sh.n_owned == 0:
            self._du = None
            return self.x0.new_empty((0, self.packs.latent))
        self._du = du1, du2 = self.round_backward(i)
        shape = (sh.n_ghost, self.packs.latent)
        if self._ghost is None or tuple(self._ghost.shape) != shape or self._ghost.device != du2.device:
            self._ghost = torch.empty(shape, dtype=torch.float32, device=du2.device)
        if sh.n_ghost:
            ops.aggregate_csr(du2, self._csr, out=self._ghost, row_range=(sh.n_owned, sh.n_local))
        return self._ghost

    def round_backward_owned(self, i: int) -> None:
        """Step 4 (runs under the reverse exchange): ``dx <- dx + du1 + A^T du2`` on the owned rows."""
        if self.sh.n_owned == 0:
            return
        du1, du2 = self._du
        self._du = None
        ops.aggregate_csr(du2, self._csr, out=self.dx, add1=self.dx, add2=du1, row_range=(0, self.sh.n_owned))
        self.xs[i + 1] = None

    def round_backward_return(self, ret: torch.Tensor) -> None:
        """Step 5: the gradient rows the peers returned, added into ``dx`` at the rows they had requested."""
        if ret.shape[0]:
            ops.halo_return_add(self.dx, ret, *self._plan)

    # -- one step through a process group ----------------------------------------------------------------------------
    def run_forward(self, x0: Optional[torch.Tensor] = None):
        """Encoder, rounds with the exchange hidden behind the interior receivers, decoders: ``(acc, temp_rate)``."""
        self.encode(x0)
        _exchange_rounds(self.halo, len(self.packs.rounds), self.stage, self.round_nodes, 0 < self.sh.n_interior)
        return self.decode()

    def run_backward(self, d_acc, d_tr, need_dx0: bool = True):
        """-> (dx0 of the owned rows, global parameter gradients in ``TrainPacks.params()`` order)."""
        self.decode_backward(d_acc, d_tr)
        for i in range(len(self.packs.rounds) - 1, -1, -1):
            handle = self.halo.start_return(self.round_backward_local(i))
            self.round_backward_owned(i)
            self.round_backward_return(self.halo.finish_return(handle))
        dx0 = self.encode_backward(need_dx0)
        grads = self.local_grads()
        self.xs = self.aggs = None
        return dx0, _all_reduce_grads(grads, self.group)

    def __call__(self, x0: Optional[torch.Tensor] = None) -> dict:
        """Differentiable predictions of the owned particles (local order; ``shard.owned_global`` maps them back).  The
        backward leaves the global gradient in every node-stream parameter's ``.grad``; edge-model parameters keep
        ``grad = None``, as on one GPU."""
        x = self.sh.x_feat if x0 is None else x0
        self._prepare(x.detach().float())
        acc, tr = _ShardedNodeStream.apply(self, x, *self.packs.params())
        return {"acceleration": acc, "temp_rate": tr}


class _ShardedNodeStream(torch.autograd.Function):
    """``acceleration, temp_rate`` of the owned rows = f(x0 owned; node-stream parameters) over a process group."""

    @staticmethod
    def forward(ctx, runner: ShardedTraining, x0: torch.Tensor, *params: torch.Tensor):
        ctx.runner = runner
        return runner.run_forward(x0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_acc, d_tr):
        runner = ctx.runner
        ctx.runner = None
        dx0, grads = runner.run_backward(d_acc, d_tr, ctx.needs_input_grad[1])
        return (None, dx0, *grads)


# ----------------------------------------------------------------------------
# sharded training (message_source="edge", model.train_edge_messages)
# ----------------------------------------------------------------------------

def edge_split_rows(n_interior: int, k: int, tile: int = 32) -> int:
    """Receivers of an edge-mode round's interior part: ``n_interior`` rounded DOWN so that ``n_split * k`` is a multiple of
    ``tile``, so that the TILED32 edge tensors split at a tile boundary; 0 when no positive count aligns."""
    if n_interior < 0 or k < 1 or tile < 1:
        raise ValueError(f"edge_split_rows: n_interior {n_interior}, k {k}, tile {tile}")
    step = tile // math.gcd(k, tile)
    return n_interior - n_interior % step


def shard_edge_training_bytes(n_owned: int, n_ghost: int, k: int, latent: int, hidden: int, num_hidden_layers: int,
                              rounds: int) -> int:
    """One rank's share of the edge-mode training memory: ``training.edge_training_bytes`` over the shard's
    ``n_owned * k`` edges, plus the node tables kept per round with their ghost rows (``L n_local D`` floats)."""
    return training.edge_training_bytes(n_owned * k, latent, hidden, num_hidden_layers, rounds) + \
        4 * rounds * (n_owned + n_ghost) * latent


class ShardedEdgeTraining(ShardedTraining, training.EdgeStreamSteps):
    """A training step of an ``EncodeProcessDecode`` with ``message_source="edge"`` and ``model.train_edge_messages`` over
    one spatial tile: the pieces of :class:`training.EdgeStreamSteps`, which :class:`training._EdgeStreams` runs over a
    whole graph, on the shard's local rows (``ShardedTraining(model, shard)`` returns one for such a model).  Here is
    only what a tile adds: ghost rows behind the owned ones in every table, two receiver ranges around the forward
    exchange, the ``dPs`` rows that cross ranks, and the rank that owns nothing (guarded here and in
    :class:`ShardedTraining`, never inside the pieces).

    Forward of round i: ``x_i`` sits in the owned rows of the kept local table ``[owned | ghosts]`` (:meth:`stage`), the
    exchange fills the ghosts.  Under it the interior part projects the owned rows and runs receivers ``[0, n_split)``;
    after it the boundary part projects the ghosts and runs ``[n_split, n_owned)``.  ``n_split``
    (:func:`edge_split_rows`) puts the split on a 32-edge tile.

    Backward of round i: the step up to dh1 of every local edge; ``dPs`` of the ghost senders into the send buffer (a
    ghost row reaches the loss only through its ``Ps`` row, so ``dPs``, H wide, is what crosses ranks); under the
    reverse exchange the edge-row reductions, ``dPs`` of the owned rows and ``dPd``; then the returned rows are added
    into ``dPs`` (``ops.halo_return_add``) and the step finishes the round.  One all-reduce sums the parameter
    gradients in ``EdgeTrainPacks.params()`` order."""

    def __init__(self, model, shard: Shard, halo=None, group=None):
        super().__init__(model, shard, halo, group)
        self.n_split = edge_split_rows(shard.n_interior, shard.k)
        self.d_edge_attr = None

    # -- set-up ------------------------------------------------------------------------------------------------------
    def _prepare(self, x0: torch.Tensor, edge_attr: Optional[torch.Tensor] = None) -> None:
        m, sh = self.model, self.sh
        ea = sh.edge_attr if edge_attr is None else edge_attr
        with torch.no_grad():
            m._materialize_all(x0.shape[1], ea.shape[1])
            D, H, nh, L = m._latent_size, m._mlp_hidden_size, m._mlp_num_hidden_layers, len(m.processor)
            need = shard_edge_training_bytes(sh.n_owned, sh.n_ghost, sh.k, D, H, nh, L)
            free = training.free_device_bytes(x0.device)
            if need > free:
                raise CgnnError(f"rank {sh.rank}: edge-mode training needs about {need / 2**30:.1f} GiB of device memory for "
                                f"the edge latents of every round, the edge-row backward scratch and the local node tables "
                                f"({sh.n_owned * sh.k} local edges, {sh.n_local} local rows, latent {D}, hidden {H}, {L} "
                                f"rounds); {free / 2**30:.1f} GiB are free")
            self.packs = m._train_packs(edge=True)      # refuses what the edge training kernels do not take (CgnnError)
        if self._csr is None and sh.n_owned:
            self._csr = ops.SenderCsr(sh.src_local, None, sh.n_local)      # the local edges by sender, once per shard
            self._plan = halo_return_plan(sh.send_idx.to(x0.device), sh.send_counts, sh.n_owned)

    # -- forward pieces ----------------------------------------------------------------------------------------------
    def encode(self, x0: Optional[torch.Tensor] = None, edge_attr: Optional[torch.Tensor] = None) -> None:
        """Node encoder on the owned rows, edge encoder on the local edges (defaults: ``shard.x_feat`` /
        ``shard.edge_attr``)."""
        sh = self.sh
        x0 = (sh.x_feat if x0 is None else x0).detach().float().contiguous()
        ea = (sh.edge_attr if edge_attr is None else edge_attr).detach().float().contiguous()
        if x0.shape[0] != sh.n_owned or ea.shape[0] != sh.n_owned * sh.k:
            raise CgnnError(f"ShardedTraining: {x0.shape[0]} input rows and {ea.shape[0]} edges for {sh.n_owned} owned "
                            f"particles with k = {sh.k}")
        self._prepare(x0, ea)
        if sh.n_owned == 0:         # no rows, no edges, no ghosts: nothing to encode
            self.x0, self.edge_attr = x0, ea
            self.xs, self.es, self.aggs = [x0.new_empty((0, self.packs.latent))], [], []
            return
        self._encode(self.packs, x0, ea, sh.src_local, sh.dst_local, sh.k, sh.n_local)

    def stage(self, i: int) -> torch.Tensor:
        """Round ``i``'s local table, kept for the backward: ``x_i`` is in its owned rows, the exchange is to fill the
        ghost rows.  Makes room for the round's results."""
        if self.sh.n_owned == 0:
            self.xs.append(self.x0.new_empty((0, self.packs.latent)))
        else:
            self._new_round()
        return self.xs[i]

    def round_nodes(self, i: int, part: str = "all") -> None:
        """Round ``i`` for the owned receivers of ``part``: ``"interior"`` ([0, n_split): no ghost sender, may run under
        the exchange; projects the owned rows), ``"boundary"`` (after it; projects the ghost rows) or ``"all"``."""
        sh = self.sh
        no = sh.n_owned
        if no == 0:
            return
        a, b = {"all": (0, no), "interior": (0, self.n_split), "boundary": (self.n_split, no)}[part]
        if part != "boundary":
            self._project(i, 0, no)
        if part != "interior" and sh.n_ghost:
            self._project(i, no, sh.n_local)
        if b > a:
            self._round_forward(i, a, b)

    # -- backward pieces ---------------------------------------------------------------------------------------------
    def round_backward_local(self, i: int) -> torch.Tensor:
        """Round ``i`` up to dh1 of every local edge, then ``dPs`` of the ghost senders, written into (and returned as) the
        send buffer of the reverse exchange, [n_ghost, H]."""
        sh, H = self.sh, self.packs.hidden
        self._round = i
        if sh.n_owned == 0:
            return self.x0.new_empty((0, H))
        g_a0 = self._round_backward_edges(i)
        if self._ghost is None or tuple(self._ghost.shape) != (sh.n_ghost, H) or self._ghost.device != g_a0.device:
            self._ghost = torch.empty((sh.n_ghost, H), dtype=torch.float32, device=g_a0.device)
        if sh.n_ghost:
            ops.aggregate_csr(g_a0, self._csr, out=self._ghost, row_range=(sh.n_owned, sh.n_local))
        return self._ghost

    def round_backward_owned(self, i: int) -> None:
        """Runs under the reverse exchange: the edge-row reductions, ``dPs`` of the owned rows and ``dPd``."""
        if self.sh.n_owned:
            self._round_backward_sums(i, self._csr)

    def round_backward_return(self, ret: torch.Tensor) -> None:
        """The ``dPs`` rows the peers returned, added at the rows they had requested; then the round's finish."""
        if self.sh.n_owned == 0:
            return
        if ret.shape[0]:
            ops.halo_return_add(self._dps, ret, *self._plan)
        self._round_backward_finish(self._round)

    def encode_backward(self, need_dx0: bool = True, need_dea: bool = False) -> Optional[torch.Tensor]:
        dx0 = super().encode_backward(need_dx0, need_dea=need_dea)
        if self.sh.n_owned == 0:
            self.d_edge_attr = torch.zeros_like(self.edge_attr) if need_dea else None
        return dx0

    # -- one step through a process group ----------------------------------------------------------------------------
    def run_forward(self, x0: Optional[torch.Tensor] = None, edge_attr: Optional[torch.Tensor] = None):
        """Encoders, rounds with the exchange hidden behind the interior receivers, decoders: ``(acc, temp_rate)``."""
        self.encode(x0, edge_attr)
        _exchange_rounds(self.halo, len(self.packs.rounds), self.stage, self.round_nodes, 0 < self.n_split)
        return self.decode()

    def run_backward(self, d_acc, d_tr, need_dx0: bool = True, need_dea: bool = False):
        """-> (dx0 of the owned rows, d edge_attr of the local edges or None, global parameter gradients in
        ``EdgeTrainPacks.params()`` order)."""
        self.decode_backward(d_acc, d_tr)
        for i in range(len(self.packs.rounds) - 1, -1, -1):
            handle = self.halo.start_return(self.round_backward_local(i))
            self.round_backward_owned(i)
            self.round_backward_return(self.halo.finish_return(handle))
        dx0 = self.encode_backward(need_dx0, need_dea)
        grads = self.local_grads()
        self.xs = self.aggs = self.es = None
        return dx0, self.d_edge_attr, _all_reduce_grads(grads, self.group)

    def __call__(self, x0: Optional[torch.Tensor] = None, edge_attr: Optional[torch.Tensor] = None) -> dict:
        """Differentiable predictions of the owned particles (local order).  The backward leaves the global gradient in
        every parameter's ``.grad``, the edge models' included, and ``d edge_attr`` of the local edges in the edge
        features' ``.grad`` when they require one (default: ``shard.edge_attr``)."""
        x = self.sh.x_feat if x0 is None else x0
        ea = self.sh.edge_attr if edge_attr is None else edge_attr
        self._prepare(x.detach().float(), ea)
        acc, tr = _ShardedEdgeStreams.apply(self, x, ea, *self.packs.params())
        return {"acceleration": acc, "temp_rate": tr}


class _ShardedEdgeStreams(torch.autograd.Function):
    """``acceleration, temp_rate`` of the owned rows = f(x0 owned, edge_attr local; all parameters) over a process group."""

    @staticmethod
    def forward(ctx, runner: ShardedEdgeTraining, x0: torch.Tensor, edge_attr: torch.Tensor, *params: torch.Tensor):
        ctx.runner = runner
        return runner.run_forward(x0, edge_attr)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_acc, d_tr):
        runner = ctx.runner
        ctx.runner = None
        dx0, dea, grads = runner.run_backward(d_acc, d_tr, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return (None, dx0, dea, *grads)


# ----------------------------------------------------------------------------
# sharded rollout (reference render_rollout.rollout over spatial tiles)
# ----------------------------------------------------------------------------

def _world_of(group=None) -> Tuple[int, int]:
    """``(world, rank)`` of the group; a world of one when no process group is up."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def rollout_arguments(data: dict, window_size: int, num_neighbors: int, num_steps: Optional[int]):
    """Checks a rollout's arguments before any device work; returns ``(coords, energy [T, N, 1], total_time)`` with
    ``total_time`` the frame count ``rollout.rollout`` produces."""
    coords, energy = data["Coordinates"], data["InternalEnergy"]
    if energy.dim() == 2:
        energy = energy.unsqueeze(-1)
    if window_size < 2:
        raise ValueError(f"sharded rollout: window_size {window_size} < 2 (velocities need two frames)")
    if coords.dim() != 3 or coords.shape[2] != 3 or energy.dim() != 3 or tuple(energy.shape[:2]) != tuple(coords.shape[:2]):
        raise ValueError(f"sharded rollout: Coordinates [T, N, 3] and InternalEnergy [T, N(, 1)], got "
                         f"{tuple(coords.shape)} / {tuple(data['InternalEnergy'].shape)}")
    n = coords.shape[1]
    if coords.shape[0] < window_size:
        raise ValueError(f"sharded rollout: {coords.shape[0]} frames, fewer than the window of {window_size}")
    if num_neighbors < 1 or num_neighbors > n:
        raise ValueError(f"sharded rollout: num_neighbors {num_neighbors} outside [1, {n}] (N = {n})")
    if n >= 2 ** 31:
        raise ValueError("sharded rollout: more than 2^31 - 1 particles (ids travel as int32)")
    if num_steps is not None and num_steps < 0:
        raise ValueError(f"sharded rollout: num_steps {num_steps} < 0")
    total = coords.shape[0] if num_steps is None else window_size + num_steps
    return coords, energy, total


def rollout_capacity(owner: torch.Tensor, world: int) -> Tuple[List[int], int]:
    """``(owned count of every rank, cap = the largest)`` from the replicated owner of every particle: every rank knows
    every rank's count, hence the common send-block size, without a collective."""
    counts = torch.bincount(owner.reshape(-1).long(), minlength=world)
    if counts.numel() != world:
        raise CgnnError(f"rollout_capacity: owners outside [0, {world})")
    counts = counts.tolist()
    return counts, max(counts)


def _step_capacity(sh: Shard, world: int) -> Tuple[List[int], int]:
    """``(owned count of every rank, cap)`` of a step's shard: the common send-block size is the largest owned count,
    known on every rank from the replicated owner map without a collective."""
    if sh._counts is not None:      # the balanced plan on the device: cgnn_tile_classify counted every rank's rows
        counts = sh._counts.tolist()
    else:
        counts, _ = rollout_capacity(sh._owner, world)
    if counts[sh.rank] != sh.n_owned:
        raise CgnnError(f"rank {sh.rank}: {sh.n_owned} owned particles, the owner map says {counts[sh.rank]}")
    return counts, max(counts)


def window_checksum(coords_w: torch.Tensor, energy_w: torch.Tensor) -> torch.Tensor:
    """float64 [4] fingerprint of an initial window (plain and position-weighted sums, frame by frame), computed on the
    window's own device; non-finite sums are mapped to fixed values so that equal data compare equal."""
    out = []
    for t in (coords_w, energy_w):
        s1 = torch.zeros((), dtype=torch.float64, device=t.device)
        s2 = torch.zeros((), dtype=torch.float64, device=t.device)
        w = None
        for f in range(t.shape[0]):
            x = t[f].reshape(-1).double()
            if w is None:
                w = torch.arange(x.numel(), dtype=torch.float64, device=t.device).remainder_(1021).add_(1.0)
            s1 += x.sum()
            s2 += (x * w).sum() * float(f + 1)
        out += [s1, s2]
    return torch.nan_to_num(torch.stack(out), nan=-1.0, posinf=1e300, neginf=-1e300)


def _all_reduce_max_(t: torch.Tensor, group=None) -> torch.Tensor:
    import torch.distributed as dist
    if not _group_up():
        return t
    return _collective(dist.all_reduce, t, op=dist.ReduceOp.MAX, group=group)()


def check_same_data(coords_w: torch.Tensor, energy_w: torch.Tensor, device, group=None) -> None:
    """One all-reduce (MAX of the checksum and of its negation): every rank raises ``ValueError`` together when the
    ranks' initial windows differ, instead of running apart into mismatched collectives."""
    c = window_checksum(coords_w, energy_w).to(device)
    both = _all_reduce_max_(torch.cat([c, -c]), group).cpu()
    hi, lo = both[:4], -both[4:]
    if not torch.equal(hi, lo):
        raise ValueError("sharded rollout: the ranks passed different data (initial-window checksums differ)")


def all_gather_rows(block: torch.Tensor, group=None) -> torch.Tensor:
    """``[world * cap, W]``: every rank's ``[cap, W]`` block in rank order (one ``all_gather_into_tensor``)."""
    import torch.distributed as dist
    out = torch.empty((dist.get_world_size(group) * block.shape[0], block.shape[1]), dtype=block.dtype,
                      device=block.device)
    return _collective(dist.all_gather_into_tensor, out, block.contiguous(), group=group)()


class ShardedRollout:
    """One rank's part of a rollout over spatial tiles.  The trajectory ``[T, N, 3]`` / ``[T, N, 1]`` is replicated on
    every rank (as ``rollout.rollout`` holds it); ownership is recomputed from each step's last frame, so a particle
    that crossed a tile plane belongs to its new tile from the next step on and nothing per particle has to move.

    A step ``t`` is five pieces, separate so that one process can interleave several ranks (tests):

    1. :meth:`plan`: the wrapped last frame of all N particles (``cgnn_window_features``' bits, what ``preprocess``
       hands the k-NN) -> :func:`build_shard`, every rank's owned count and the send-block capacity ``cap``; the caller
       then completes the ghost plan (:func:`exchange_requests` or :func:`finish_shard`);
    2. :meth:`features`: the owned rows' node features straight from the window ``traj[t-W:t]``
       (``cgnn_window_features_rows``);
    3. :meth:`forward`: a :class:`ShardedForward` with the given halo;
    4. :meth:`integrate`: ``cgnn_rollout_integrate`` -> the send block ``[cap, ROLLOUT_ROW]`` (padding id -1);
    5. :meth:`publish`: the gathered ``[world * cap, ROLLOUT_ROW]`` rows -> frame ``t`` (``cgnn_frame_unpack``).

    Buffers that depend on the owned count are made per step.  ``decomposition``: as in :func:`build_shard`; with
    ``"balanced"`` the planes follow the particles from step to step and ``cap`` stays near ``N / world``.
    ``knn_grid``, ``min_image_edge_attr``: as in :func:`build_shard`, for every step's search."""

    def __init__(self, model, data: dict, metadata: dict, dt: float, box_size: float, window_size: int = 6,
                 num_neighbors: int = 16, num_steps: Optional[int] = None, device=None, world: int = 1, rank: int = 0,
                 decomposition: str = "uniform", *, min_image_edge_attr: bool = False, knn_grid: str = "uniform"):
        self.knn_grid = ops.check_knn_grid(knn_grid, "sharded rollout")
        self.min_image_edge_attr = ops.check_min_image(min_image_edge_attr, "sharded rollout")
        coords, energy, total = rollout_arguments(data, window_size, num_neighbors, num_steps)
        if decomposition not in DECOMPOSITIONS:
            raise ValueError(f"sharded rollout: decomposition {decomposition!r}; known: {DECOMPOSITIONS}")
        self.decomposition = decomposition
        if not 0 <= rank < world:
            raise ValueError(f"sharded rollout: rank {rank} outside a world of {world}")
        if device is None:
            device = next(model.parameters()).device
        self.device = torch.device(device)
        self.model, self.world, self.rank = model, world, rank
        self.W, self.k, self.total_time = window_size, int(num_neighbors), total
        self.n = coords.shape[1]
        self.dt, self.box = float(dt), float(box_size)
        self.meta = dict(metadata)
        self.meta["dt"], self.meta["box_size"] = dt, box_size
        self.stats = ops.integration_stats(self.meta)
        # NaN until published: a particle no rank delivered cannot pass for a result
        self.pos = torch.full((total, self.n, 3), float("nan"), dtype=torch.float32, device=self.device)
        self.tmp = torch.full((total, self.n, 1), float("nan"), dtype=torch.float32, device=self.device)
        self.pos[:window_size] = coords[:window_size].to(self.device).float()
        self.tmp[:window_size] = energy[:window_size].to(self.device).float()
        self.counts: List[int] = []
        self.cap = 0

    def plan(self, t: int) -> Shard:
        """Step ``t``'s shard (no send plan yet) from the wrapped frame ``t - 1``; sets ``counts`` and ``cap``."""
        _, recent = ops.window_features(self.pos[t - 2:t], self.tmp[t - 2:t], self.meta, self.dt, self.box)
        if not bool(torch.isfinite(recent).all()):        # the neighbour search must never see a NaN position
            raise CgnnError(f"sharded rollout: frame {t - 1} holds non-finite positions (rows that were never published, "
                            f"or a diverged model)")
        sh = build_shard(recent, self.box, self.k, self.world, self.rank, decomposition=self.decomposition,
                         knn_grid=self.knn_grid, min_image_edge_attr=self.min_image_edge_attr)
        self.counts, self.cap = _step_capacity(sh, self.world)
        return sh

    def features(self, sh: Shard, t: int) -> torch.Tensor:
        sh.x_feat, _ = ops.window_features_rows(self.pos[t - self.W:t], self.tmp[t - self.W:t], sh.owned_global,
                                                self.meta, self.dt, self.box)
        return sh.x_feat

    def forward(self, sh: Shard, halo: Optional[Callable] = None) -> ShardedForward:
        return ShardedForward(self.model, sh, halo)

    def integrate(self, sh: Shard, pred: dict, t: int) -> torch.Tensor:
        if sh.n_owned == 0:        # an empty rank sends padding rows only
            block = torch.zeros((self.cap, _lib.ROLLOUT_ROW), dtype=torch.float32, device=self.device)
            block.view(torch.int32)[:, _lib.ROLLOUT_ROW - 1] = -1
            return block
        return ops.rollout_integrate(pred["acceleration"], pred["temp_rate"], self.pos[t - 2], self.pos[t - 1],
                                     self.tmp[t - 1], sh.owned_global, self.meta, n_out=self.cap, stats=self.stats)

    def publish(self, rows: torch.Tensor, t: int) -> None:
        ops.frame_unpack(rows, self.pos[t], self.tmp[t])

    def result(self) -> dict:
        return {"Coordinates": self.pos, "InternalEnergy": self.tmp}


def sharded_rollout(model, data: dict, metadata: dict, noise_std: float, dt: float, box_size: float,
                    window_size: int = 6, num_neighbors: int = 16, num_steps: Optional[int] = None, device=None,
                    group=None, decomposition: str = "uniform", storage: str = "replicated", *,
                    min_image_edge_attr: bool = False, knn_grid: str = "uniform") -> dict:
    """``rollout.rollout`` over the ranks of ``group`` (a world of one when no process group is up): same arguments,
    return value and frame count, and the same bits.  Every rank passes the same ``data`` (checked once, by one
    all-reduce of a checksum) and returns the whole trajectory.  ``noise_std`` is ignored, as there.
    ``decomposition``, ``knn_grid``: as in :func:`build_shard`; they change who computes a row and how its neighbours
    are found, never the row.  ``min_image_edge_attr``: as in ``rollout.rollout``, for both storages.

    Per step: the shard of the wrapped last frame, the ghost-id all-to-all, the forward with one halo all-to-all per
    round, the integration of the owned particles and one all-gather of the packed rows into the next frame.

    ``storage="owned"``: every rank keeps and returns only the particles it holds (:class:`MigratingRollout`):
    ``{"frames": [rows_0, ..., rows_{T-1}], "n_total": N, "world": w, "rank": r}``, ``rows_t [n_held_t, ROLLOUT_ROW]``
    the packed rows (x, y, z, temperature, int32 id bits) of the particles this rank held at frame t; the first
    ``window_size`` frames are its initially owned particles (``owner_of`` of the wrapped frame W-1), stored raw.
    After start-up, which slices the given window, nothing of length N exists on any rank; a particle that crosses a
    tile plane is sent to its new rank with its window history.  The same frames and bits
    (:func:`assemble_frames`, :func:`owned_frame_errors`).  With ``decomposition="balanced"`` the planes are those of
    the initial frame and stay fixed for the run: re-balancing needs a distributed quantile search and is not built.
    At most 64 ranks."""
    del noise_std
    ops.check_knn_grid(knn_grid, "sharded_rollout")
    ops.check_min_image(min_image_edge_attr, "sharded_rollout")
    rollout_arguments(data, window_size, num_neighbors, num_steps)
    world, rank = _world_of(group)
    check_rollout_storage(storage, world, "sharded_rollout")
    if storage == "owned":
        if decomposition not in DECOMPOSITIONS:
            raise ValueError(f"sharded rollout: decomposition {decomposition!r}; known: {DECOMPOSITIONS}")
        if device is None:
            device = next(model.parameters()).device
        model.eval()
        with torch.no_grad():
            return _owned_rollout(model, data, metadata, dt, box_size, window_size, num_neighbors, num_steps,
                                  torch.device(device), group, decomposition, knn_grid, min_image_edge_attr)
    import torch.distributed as dist
    distributed = dist.is_available() and dist.is_initialized()
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    model.eval()
    with torch.no_grad():
        if distributed:
            energy = data["InternalEnergy"]
            check_same_data(data["Coordinates"][:window_size], energy[:window_size], device, group)
        runner = ShardedRollout(model, data, metadata, dt, box_size, window_size, num_neighbors, num_steps, device,
                                world, rank, decomposition, knn_grid=knn_grid,
                                min_image_edge_attr=min_image_edge_attr)
        for t in range(window_size, runner.total_time):
            sh = runner.plan(t)
            if distributed:
                sh = exchange_requests(sh, group)
                halo = HaloExchange(sh, group)
            else:
                sh = finish_shard(sh, sh.want_global)
                halo = lambda table: None      # noqa: E731  (a world of one has no ghosts)
            runner.features(sh, t)
            pred = runner.forward(sh, halo)()
            block = runner.integrate(sh, pred, t)
            runner.publish(all_gather_rows(block, group) if distributed else block, t)
    return runner.result()


# ----------------------------------------------------------------------------
# sharded rollout with particle migration (storage="owned"): every rank keeps only its tile
# ----------------------------------------------------------------------------

ROLLOUT_STORAGE = ("replicated", "owned")
MAX_MIGRATING_WORLD = _lib.MIGRATE_MAX_WORLD      # a held row's peer mask is one 64-bit word


def check_rollout_storage(storage: str, world: int, what: str = "sharded rollout") -> str:
    if storage not in ROLLOUT_STORAGE:
        raise ValueError(f"{what}: storage {storage!r}; known: {ROLLOUT_STORAGE}")
    if storage == "owned" and world > MAX_MIGRATING_WORLD:
        raise ValueError(f"{what}: storage='owned' supports at most {MAX_MIGRATING_WORLD} ranks (the per-particle peer "
                         f"mask is one 64-bit word), got a world of {world}")
    return storage


def first_margin(box_size: float, k: int, n_total: int, margin_factor: float = 2.0) -> float:
    """:func:`build_shard`'s first search margin: ``margin_factor`` x the radius that holds k particles at mean density."""
    return margin_factor * box_size * (3.0 * k / (4.0 * 3.141592653589793 * max(n_total, 1))) ** (1.0 / 3.0)


def peer_mask(pos: torch.Tensor, box_size: float, world: int, rank: int, margin: float,
              planes: Optional[TilePlanes] = None) -> torch.Tensor:
    """bool ``[n, world]``: column p marks the rows of ``pos`` (positions rank ``rank`` holds) that peer p's search needs
    for ``margin``: those within the margin of p's tile, one test per tile (:func:`_near_tile`, not one per periodic
    image, so nothing is marked twice).  The rank's own column stays empty.  The torch restatement of
    ``cgnn_halo_select``."""
    out = torch.zeros((pos.shape[0], world), dtype=torch.bool, device=pos.device)
    for p in range(world):
        if p != rank:
            lo, hi = tile_bounds(box_size, world, p, planes)
            out[:, p] = _near_tile(pos, box_size, lo, hi, margin)
    return out


def subset_shard(rank: int, world: int, k: int, owned_s: torch.Tensor, senders_s: torch.Tensor, edge_attr: torch.Tensor,
                 owner_sub: torch.Tensor, sub_ids: Optional[torch.Tensor] = None) -> Shard:
    """:func:`build_shard`'s tail in subset space, with nothing of length N: the search set has ``n_sub`` rows in
    ascending global id (``sub_ids`` int64; ``None``: the set is the whole box and a row is its id), ``owner_sub`` is
    the rank holding each, ``owned_s`` the subset rows of the queries (the rank's own particles, in the local order
    wanted) and ``senders_s [n_owned * k]`` their neighbours as subset rows.  Interior receivers first, ghosts grouped
    by the rank they came from in ascending id, local numbering ``[owned | ghosts]``: every field as
    :func:`build_shard` makes it.  The send plan comes from :func:`finish_shard_by_search`."""
    dev = owner_sub.device
    n_sub = owner_sub.numel()
    owned = owned_s.long()
    n_owned = owned.numel()
    senders = senders_s.long()
    remote = owner_sub[senders] != rank
    is_boundary = remote.view(n_owned, k).any(dim=1) if n_owned else remote.new_zeros((0,))
    n_interior = int((~is_boundary).sum())
    if 0 < n_interior < n_owned:
        regroup = torch.cat([torch.nonzero(~is_boundary).squeeze(1), torch.nonzero(is_boundary).squeeze(1)])
        owned = owned[regroup]
        senders = senders.view(n_owned, k)[regroup].reshape(-1)
        edge_attr = edge_attr.view(n_owned, k, -1)[regroup].reshape(n_owned * k, -1).contiguous()
        remote = remote.view(n_owned, k)[regroup].reshape(-1)
    ghosts = torch.unique(senders[remote])
    g_owner = owner_sub[ghosts].long()
    perm = torch.argsort(g_owner * max(n_sub, 1) + ghosts)       # by rank, ascending subset row (= ascending id) inside
    ghosts, g_owner = ghosts[perm], g_owner[perm]
    recv_counts = torch.bincount(g_owner, minlength=world).tolist()
    s2l = torch.full((n_sub,), -1, dtype=torch.int32, device=dev)
    s2l[owned] = torch.arange(n_owned, dtype=torch.int32, device=dev)
    s2l[ghosts] = n_owned + torch.arange(ghosts.numel(), dtype=torch.int32, device=dev)
    src_local = s2l[senders].contiguous()
    dst_local = torch.arange(n_owned, dtype=torch.int32, device=dev).repeat_interleave(k)
    own_sorted = torch.sort(owned).values
    if sub_ids is None:
        owned_global, ghost_global, held_sorted = owned, ghosts, own_sorted
    else:
        owned_global, ghost_global, held_sorted = sub_ids[owned], sub_ids[ghosts], sub_ids[own_sorted]
    sh = Shard(rank, world, k, n_owned, ghosts.numel(), owned_global, ghost_global, src_local, dst_local, edge_attr,
               recv_counts, want_global=list(torch.split(ghost_global, recv_counts)), n_interior=n_interior)
    sh._s2l = s2l                             # subset row -> local row (-1: neither owned nor a ghost)
    sh._held_sorted = held_sorted             # the held global ids, ascending
    sh._local_of_sorted = s2l[own_sorted]     # ... and the local row of each
    return sh


def held_rows_of(held_sorted: torch.Tensor, local_of_sorted: torch.Tensor, request: torch.Tensor, what: str) -> torch.Tensor:
    """Local rows of the requested global ids, by a search in the ascending held ids; raises on an id not held."""
    req = request.long()
    if req.numel() == 0:
        return local_of_sorted[:0]
    if held_sorted.numel() == 0:
        raise RuntimeError(f"{what} requested rows this rank does not own")
    at = torch.searchsorted(held_sorted, req).clamp_(max=held_sorted.numel() - 1)
    if not bool((held_sorted[at] == req).all()):
        raise RuntimeError(f"{what} requested rows this rank does not own")
    return local_of_sorted[at]


def finish_shard_by_search(sh: Shard, requests_from_peers: Sequence[torch.Tensor]) -> Shard:
    """:func:`finish_shard` for a :func:`subset_shard`: the requested global ids are found in the sorted held ids (no
    ``[n_total]`` map)."""
    idx = [held_rows_of(sh._held_sorted, sh._local_of_sorted, req, f"rank {sh.rank}: rank {r}")
           for r, req in enumerate(requests_from_peers)]
    sh.send_counts = [int(t.numel()) for t in idx]
    sh.send_idx = torch.cat(idx).to(torch.int32).contiguous() if idx else torch.empty(0, dtype=torch.int32)
    return sh


class MigratingRollout:
    """One rank's part of a rollout over spatial tiles that holds this rank's particles only (``storage="owned"``).
    It is built from the rank's own rows -- ``ids`` (global ids), ``coords_w [W, n_own, 3]`` and ``energy_w [W, n_own(,
    1)]``, the initial window of those particles -- and the integer ``n_total``; no tensor of length N is passed in or
    made afterwards.  The frames and bits are those of ``rollout.rollout``.

    State: the window histories in a frame-major ring ``hist [W, cap, 4]`` of (x, y, z, T) (frame f in slot f mod W: the
    same phase on every rank), ``ids int32 [cap]``, a second ring of the same size that migration gathers into, and the
    recorded frame blocks (``[n_held_t, ROLLOUT_ROW]`` each): ``n_held * (16 W + 4)`` bytes per ring plus ``20 n_held``
    per recorded frame.

    A step is these pieces, separate so that one process can interleave several ranks (tests); ``sharded_rollout``
    joins them with the collectives:

    1. :meth:`begin`: wrapped last positions of the held rows from the ring (``cgnn_history_features``);
    2. :meth:`halo_out`: ``(x, y, z, id)`` rows for every peer whose tile, grown by the margin, holds them
       (``cgnn_halo_select`` / ``cgnn_halo_pack``), one all-to-all-v;
    3. :meth:`search`: held rows + imports sorted by global id (:func:`build_shard`'s ``sub`` for that margin), the
       owned queries through ``ops.knn_periodic``, the k-th neighbour checked against the margin; returns "my check
       failed": after a MAX all-reduce all ranks :meth:`widen` (double the margin) and repeat 2-3 together;
    4. :meth:`number` (:func:`subset_shard`), then the ghost-id exchange with :func:`finish_shard_by_search`;
    5. :meth:`features` and :meth:`forward` (an unchanged :class:`ShardedForward`);
    6. :meth:`advance`: ``cgnn_rollout_advance`` integrates, writes the ring slot of the oldest frame, records the
       frame rows and counts the rows per destination rank;
    7. :meth:`migrate_out` / :meth:`receive`: leavers ``(id, W float4)`` grouped by destination, one all-to-all-v,
       stayers and arrivals gathered into the second ring (``cgnn_migrate_pack`` / ``cgnn_migrate_unpack``);
       :meth:`check_total` on the all-reduced held counts: a lost particle raises on every rank.

    ``planes``: the cutting planes of a balanced decomposition, fixed for the run (the ranks cannot re-balance without
    a distributed quantile search over all particles, which is not built); ``None``: equal-volume tiles.
    ``min_image_edge_attr``: as in :func:`build_shard`, for every search."""

    def __init__(self, model, ids: torch.Tensor, coords_w: torch.Tensor, energy_w: torch.Tensor, *, n_total: int,
                 metadata: dict, dt: float, box_size: float, window_size: int = 6, num_neighbors: int = 16,
                 num_steps: int = 0, device=None, world: int = 1, rank: int = 0, planes: Optional[TilePlanes] = None,
                 knn_grid: str = "uniform", margin_factor: float = 2.0, min_image_edge_attr: bool = False):
        what = "migrating rollout"
        self.knn_grid = ops.check_knn_grid(knn_grid, what)
        self.min_image_edge_attr = ops.check_min_image(min_image_edge_attr, what)
        check_rollout_storage("owned", world, what)
        if isinstance(n_total, torch.Tensor) or int(n_total) != n_total:
            raise ValueError(f"{what}: n_total must be an integer")
        n_total, W, k = int(n_total), int(window_size), int(num_neighbors)
        if not 2 <= W <= 32:
            raise ValueError(f"{what}: window_size {W} outside [2, 32]")
        if not 0 <= rank < world:
            raise ValueError(f"{what}: rank {rank} outside a world of {world}")
        if n_total >= 2 ** 31 or k < 1 or k > n_total or num_steps < 0:
            raise ValueError(f"{what}: n_total {n_total}, num_neighbors {k}, num_steps {num_steps}")
        if energy_w.dim() == 2:
            energy_w = energy_w.unsqueeze(-1)
        n = ids.numel()
        if coords_w.shape != (W, n, 3) or energy_w.shape != (W, n, 1):
            raise ValueError(f"{what}: the rank's window must be [W, n_own, 3] / [W, n_own(, 1)] for its {n} ids and W = "
                             f"{W}, got {tuple(coords_w.shape)} / {tuple(energy_w.shape)}")
        if planes is not None and tuple(planes.grid) != tile_grid(world):
            raise ValueError(f"{what}: planes of a {planes.grid} tile grid for a world of {world}")
        if device is None:
            device = next(model.parameters()).device
        self.device = dev = torch.device(device)
        self.model, self.world, self.rank, self.planes = model, world, rank, planes
        self.W, self.k, self.n_total, self.total_time = W, k, n_total, W + int(num_steps)
        self.dt, self.box = float(dt), float(box_size)
        self.meta = dict(metadata)
        self.meta["dt"], self.meta["box_size"] = dt, box_size
        self.stats = ops.integration_stats(self.meta)
        self.grid = tile_grid(world)
        bounds = [tile_bounds(self.box, world, r, planes) for r in range(world)]        # start-up read-backs (planes)
        self.boxes = ops.tile_boxes([b[0] for b in bounds], [b[1] for b in bounds])
        self.margin0 = first_margin(self.box, k, n_total, margin_factor)
        self.n_held = n
        self.hist, self.ids = self._ring(n)
        self.hist[:, :n, :3] = coords_w.to(dev).float()
        self.hist[:, :n, 3:] = energy_w.to(dev).float()
        self.ids[:n] = ids.to(dev).to(torch.int32)
        self._spare = None
        self.frames: List[torch.Tensor] = []
        for f in range(W):          # the initial frames, raw, in the packed row format
            rows = torch.empty((n, _lib.ROLLOUT_ROW), dtype=torch.float32, device=dev)
            rows[:, :4] = self.hist[f, :n]
            rows.view(torch.int32)[:, 4] = self.ids[:n]
            self.frames.append(rows)
        self.t = W
        self.margin, self.searches = self.margin0, 0
        self.arrivals: List[int] = []

    def _ring(self, rows: int):
        cap = rows + rows // 8 + 256
        return (torch.empty((self.W, cap, 4), dtype=torch.float32, device=self.device),     # rows >= n_held: never read
                torch.full((cap,), -1, dtype=torch.int32, device=self.device))

    @property
    def phase(self) -> int:
        return self.t % self.W

    # -- 1-3: positions, halo, search ----------------------------------------------------------------------------------
    def begin(self) -> None:
        """Step ``self.t``: the wrapped last positions (and id bits) of the held rows, storage order."""
        _, self.recent = ops.history_features(self.hist, self.n_held, self.phase, self.meta, self.dt, self.box,
                                              ids=self.ids, want_x=False, want_recent=True)
        if not bool(torch.isfinite(self.recent[:, :3]).all()):      # the neighbour search must never see a NaN position
            raise CgnnError(f"migrating rollout: rank {self.rank} holds non-finite positions at frame {self.t - 1} (a "
                            f"diverged model)")
        self.margin, self.searches = self.margin0, 0

    def widen(self) -> None:
        self.margin *= 2.0

    def halo_out(self):
        """``(rows [S, 4], send_counts)``: the held ``(x, y, z, id)`` rows every peer's search needs for the current
        margin, grouped by peer in storage order.  One read-back (the counts)."""
        mask, block_counts, counts = ops.halo_select(self.recent, self.rank, self.boxes, self.margin, self.box)
        send_counts = counts.tolist()
        starts = torch.cumsum(counts, 0) - counts
        rows = ops.halo_pack(self.recent, mask, ops.group_offsets(block_counts, starts), sum(send_counts))
        return rows, send_counts

    def search(self, imports: torch.Tensor, recv_counts: Sequence[int]) -> bool:
        """``imports [R, 4]``: the rows the peers sent, grouped by peer (``recv_counts``).  Builds the search set (held
        rows + imports in ascending global id), runs the owned queries and checks the k-th neighbours against the
        margin; returns whether the check failed (the margin must grow)."""
        self.searches += 1
        dev, n, k, rank = self.device, self.n_held, self.k, self.rank
        rows = torch.cat([self.recent, imports.to(dev)]) if imports.shape[0] else self.recent
        held_by = torch.full((n,), rank, dtype=torch.int32, device=dev)
        if imports.shape[0]:
            came = torch.repeat_interleave(torch.arange(self.world, dtype=torch.int32, device=dev),
                                           torch.tensor(list(recv_counts), device=dev))
            held_by = torch.cat([held_by, came])
        sub_ids, perm = torch.sort(rows[:, 3].contiguous().view(torch.int32).long())
        pos_sub = rows[perm, :3].contiguous()
        owner_sub = held_by[perm]
        n_sub = pos_sub.shape[0]
        if n_sub > self.n_total or (n_sub > 1 and bool((sub_ids[1:] == sub_ids[:-1]).any())):
            raise CgnnError(f"migrating rollout: rank {rank}'s search set holds a particle twice")
        whole = n_sub == self.n_total
        knn = lambda q: ops.knn_periodic(pos_sub, self.box, k, query_ids=q, want_edge_attr=True, want_order=True,   # noqa: E731
                                         grid=self.knn_grid, min_image_edge_attr=self.min_image_edge_attr)
        owned_s = torch.nonzero(owner_sub == rank).squeeze(1)
        failed = False
        if n:
            if n_sub < k:
                raise CgnnError(f"migrating rollout: rank {rank} searches {n_sub} particles for {k} neighbours")
            _, _, order = knn(owned_s[:1].to(torch.int32))
            if order is not None:
                order = order.long()
                owned_s = order[owner_sub[order] == rank]
            senders_s, edge_attr, _ = knn(owned_s.to(torch.int32))
            if not whole:
                kth = senders_s.view(-1, k)[:, k - 1].long()
                dlt = torch.abs(pos_sub[kth] - pos_sub[owned_s])
                dlt = torch.minimum(dlt, self.box - dlt)
                failed = float(dlt.norm(dim=1).max()) > self.margin
        else:
            senders_s = torch.empty(0, dtype=torch.int32, device=dev)
            edge_attr = torch.empty((0, 4), dtype=torch.float32, device=dev)
        inv = torch.empty(n_sub, dtype=torch.int64, device=dev)
        inv[perm] = torch.arange(n_sub, device=dev)
        self._found = (owned_s, senders_s, edge_attr, owner_sub, sub_ids, inv[:n])
        return failed

    # -- 4-5: numbering, features, forward -----------------------------------------------------------------------------
    def number(self) -> Shard:
        """The step's :class:`Shard` (no send plan yet) from the last :meth:`search`."""
        owned_s, senders_s, edge_attr, owner_sub, sub_ids, held_s = self._found
        self._found = None
        n = self.n_held
        sh = subset_shard(self.rank, self.world, self.k, owned_s, senders_s, edge_attr, owner_sub, sub_ids)
        self._pred_row = sh._s2l[held_s].contiguous()           # storage row -> local row (its prediction)
        sh._rows = torch.empty(n, dtype=torch.int32, device=self.device)
        sh._rows[self._pred_row.long()] = torch.arange(n, dtype=torch.int32, device=self.device)   # local -> storage
        sh._sub_ids = sub_ids
        sh.searches, sh.subset_rows = self.searches, sub_ids.numel()
        return sh

    def features(self, sh: Shard) -> torch.Tensor:
        sh.x_feat, _ = ops.history_features(self.hist, self.n_held, self.phase, self.meta, self.dt, self.box,
                                            rows=sh._rows)
        return sh.x_feat

    def forward(self, sh: Shard, halo: Optional[Callable] = None) -> ShardedForward:
        return ShardedForward(self.model, sh, halo)

    # -- 6-7: advance, migrate -------------------------------------------------------------------------------------------
    def advance(self, pred: dict) -> List[int]:
        """Integrates the held rows, writes the new frame into the ring and records it; returns the rows leaving for
        every rank (0 for this one).  One read-back (the counts)."""
        record, dest, block_counts, counts = ops.rollout_advance(
            self.hist, self.n_held, self.phase, self.ids, pred["acceleration"], pred["temp_rate"], self.meta, self.grid,
            None if self.planes is None else self.planes.tensors(), pred_row=self._pred_row, stats=self.stats)
        self.frames.append(record)
        send_counts = counts.tolist()
        self._moving = (dest, block_counts, send_counts[self.rank])
        send_counts[self.rank] = 0
        self.send_counts = send_counts
        return send_counts

    def migrate_out(self, n_arriving: int) -> torch.Tensor:
        """Stayers into the second ring (sized for the ``n_arriving`` rows to come); returns the leavers ``[S, W + 1, 4]``
        grouped by destination, storage order inside a group."""
        dest, block_counts, n_stay = self._moving
        need = n_stay + int(n_arriving)
        if self._spare is None or self._spare[0].shape[1] < need:
            self._spare = self._ring(need)
        starts, run = [], 0
        for p, c in enumerate(self.send_counts):
            starts.append(0 if p == self.rank else run)
            run += c
        offsets = ops.group_offsets(block_counts, torch.tensor(starts, dtype=torch.int64, device=self.device))
        return ops.migrate_pack(self.hist, self.n_held, self.ids, dest, self.rank, offsets, self._spare[0],
                                self._spare[1], run)

    def receive(self, arrivals: torch.Tensor) -> int:
        """Appends the arrivals behind the stayers and makes the second ring the current one; returns the held count."""
        n_stay = self._moving[2]
        arrivals = arrivals.to(self.device)
        ops.migrate_unpack(arrivals, self._spare[0], self._spare[1], n_stay)
        (self.hist, self.ids), self._spare = self._spare, (self.hist, self.ids)
        self.n_held = n_stay + arrivals.shape[0]
        self.arrivals.append(arrivals.shape[0])
        self._moving = None
        self.t += 1
        return self.n_held

    def check_total(self, held_by_all: int) -> None:
        if int(held_by_all) != self.n_total:
            raise CgnnError(f"migrating rollout: after frame {self.t - 1} the ranks hold {int(held_by_all)} particles, not "
                            f"{self.n_total}: a migration lost or duplicated rows")

    def result(self) -> dict:
        return {"frames": self.frames, "n_total": self.n_total, "world": self.world, "rank": self.rank}


def exchange_counts(send_counts: Sequence[int], device, group=None) -> List[int]:
    """All-to-all of one count per peer: what every peer is about to send this rank."""
    import torch.distributed as dist
    out = torch.tensor(list(send_counts), dtype=torch.int64, device=device)
    return _collective(dist.all_to_all_single, torch.empty_like(out), out, group=group)().tolist()


def exchange_rows(rows: torch.Tensor, send_counts: Sequence[int], recv_counts: Sequence[int], group=None) -> torch.Tensor:
    """All-to-all-v of row blocks grouped by peer (split along dim 0)."""
    import torch.distributed as dist
    recv = torch.empty((int(sum(recv_counts)),) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    return _collective(dist.all_to_all_single, recv, rows.contiguous(), output_split_sizes=list(recv_counts),
                       input_split_sizes=list(send_counts), group=group)()


def _owned_rollout(model, data: dict, metadata: dict, dt: float, box_size: float, window_size: int, num_neighbors: int,
                   num_steps: Optional[int], device, group, decomposition: str, knn_grid: str,
                   min_image_edge_attr: bool = False) -> dict:
    """``sharded_rollout(storage="owned")``: start-up slices the full initial window by the initial owner (the only place
    that touches N), then every step runs on the rank's rows."""
    import torch.distributed as dist
    coords, energy, total = rollout_arguments(data, window_size, num_neighbors, num_steps)
    world, rank = _world_of(group)
    distributed = dist.is_available() and dist.is_initialized()
    W, n_total = window_size, coords.shape[1]
    meta = dict(metadata)
    meta["dt"], meta["box_size"] = dt, box_size
    if distributed:
        check_same_data(coords[:W], energy[:W], device, group)
    _, recent = ops.window_features(coords[W - 2:W].to(device).float(), energy[W - 2:W].to(device).float(), meta, dt,
                                    box_size)
    planes = balanced_planes(recent, box_size, world) if decomposition == "balanced" else None
    own = torch.nonzero(owner_of(recent, box_size, world, planes) == rank).squeeze(1)
    del recent
    at = own.to(coords.device)
    runner = MigratingRollout(model, own, coords[:W, at], energy[:W, at], n_total=n_total, metadata=metadata, dt=dt,
                              box_size=box_size, window_size=W, num_neighbors=num_neighbors, num_steps=total - W,
                              device=device, world=world, rank=rank, planes=planes, knn_grid=knn_grid,
                              min_image_edge_attr=min_image_edge_attr)
    nobody = torch.empty((0, 4), dtype=torch.float32, device=device)
    for _ in range(W, total):
        runner.begin()
        while True:
            rows, send_counts = runner.halo_out()
            if distributed:
                recv_counts = exchange_counts(send_counts, device, group)
                failed = runner.search(exchange_rows(rows, send_counts, recv_counts, group), recv_counts)
                flag = torch.tensor([1 if failed else 0], dtype=torch.int32, device=device)
                failed = bool(_all_reduce_max_(flag, group)[0])
            else:
                failed = runner.search(nobody, [0])
            if not failed:
                break
            runner.widen()
        sh = runner.number()
        if distributed:
            sh = exchange_requests(sh, group, finish_shard_by_search)
            halo = HaloExchange(sh, group)
        else:
            sh = finish_shard_by_search(sh, sh.want_global)
            halo = lambda table: None      # noqa: E731  (a world of one has no ghosts)
        runner.features(sh)
        pred = runner.forward(sh, halo)()
        send_counts = runner.advance(pred)
        if distributed:
            recv_counts = exchange_counts(send_counts, device, group)
            leavers = runner.migrate_out(sum(recv_counts))
            held = runner.receive(exchange_rows(leavers, send_counts, recv_counts, group))
            held = int(_all_reduce_(torch.tensor([held], dtype=torch.int64, device=device), group)[0])
        else:
            leavers = runner.migrate_out(0)
            held = runner.receive(leavers[:0])
        runner.check_total(held)
    return runner.result()


def assemble_frames(results: Sequence[dict], n_total: int) -> dict:
    """The ranks' ``storage="owned"`` results -> ``{"Coordinates" [T, N, 3], "InternalEnergy" [T, N, 1]}`` on the first
    result's device (``cgnn_frame_unpack``); rows no rank delivered stay NaN.  For tests and small runs: it holds the
    whole trajectory."""
    frames = [r["frames"] for r in results]
    T = len(frames[0])
    if any(len(f) != T for f in frames):
        raise ValueError("assemble_frames: the ranks recorded different numbers of frames")
    dev = frames[0][0].device
    pos = torch.full((T, n_total, 3), float("nan"), dtype=torch.float32, device=dev)
    tmp = torch.full((T, n_total, 1), float("nan"), dtype=torch.float32, device=dev)
    for t in range(T):
        for f in frames:
            if f[t].shape[0]:
                ops.frame_unpack(f[t].to(dev), pos[t], tmp[t])
    return {"Coordinates": pos, "InternalEnergy": tmp}


def owned_frame_errors(result: dict, ground_truth: dict, group=None) -> dict:
    """``rollout.calculate_errors`` of a ``storage="owned"`` rollout without assembling it: per frame, float64 partial
    sums of the squared errors over the rows this rank recorded (the ground truth ``[T, N, 3]`` / ``[T, N(, 1)]`` is
    read at those ids), ONE all-reduce of all partial sums, then the means over N."""
    import torch.distributed as dist
    frames, n = result["frames"], int(result["n_total"])
    tc, tt = ground_truth["Coordinates"], ground_truth["InternalEnergy"]
    count = min(len(frames), len(tc), len(tt))
    dev = frames[0].device if frames else torch.device("cpu")
    sums = torch.zeros(2 * count, dtype=torch.float64, device=dev)
    for t in range(count):
        rows = frames[t]
        ids = rows[:, 4].contiguous().view(torch.int32).long()
        at = ids.to(tc.device)
        sums[t] = ((rows[:, :3].double() - tc[t][at].to(dev).double()) ** 2).sum()
        sums[count + t] = ((rows[:, 3].double() - tt[t].reshape(-1)[at.to(tt.device)].to(dev).double()) ** 2).sum()
    if dist.is_available() and dist.is_initialized():
        _all_reduce_(sums, group)
    pos = (sums[:count] / (3.0 * n)).tolist()
    tmp = (sums[count:] / float(n)).tolist()
    return {"position_errors": pos, "temperature_errors": tmp,
            "mean_position_error": sum(pos) / len(pos) if pos else None,
            "mean_temperature_error": sum(tmp) / len(tmp) if tmp else None}


# ----------------------------------------------------------------------------
# synthetic shard for bench.py (every rank regenerates the same global box from the seed)
# ----------------------------------------------------------------------------

def build_synthetic_shard(particles_per_gpu: int, world: int, rank: int, k: int, seed: int, device, metadata: dict,
                          group=None, decomposition: str = "uniform", *, min_image_edge_attr: bool = False,
                          knn_grid: str = "uniform") -> Shard:
    ops.check_knn_grid(knn_grid, "build_synthetic_shard")
    ops.check_min_image(min_image_edge_attr, "build_synthetic_shard")
    n_total = particles_per_gpu * world
    # the box of synthetic.make_snapshot(n_total, seed), bit for bit, but only one global frame (positions: ownership and the
    # neighbour search need all of them) and the feature window of the OWNED particles are built and uploaded: per rank the
    # host work is the random draws plus N + 6 N / world elements, not the whole [6, N, 3] trajectory
    snap = synthetic.LazySnapshot(n_total, seed=seed)
    box, dt = metadata["box_size"], metadata["dt"]
    W = 5
    pos = torch.remainder(snap.frame(W - 1).to(device), box).contiguous()     # the window's last frame
    sh = build_shard(pos, box, k, world, rank, decomposition=decomposition, knn_grid=knn_grid,
                     min_image_edge_attr=min_image_edge_attr)
    sh = exchange_requests(sh, group)
    coords, energy = snap.window_of(sh.owned_global)
    # node features of the owned particles: the same kernel data_utils.preprocess uses
    sh.x_feat, _ = ops.window_features(coords[:W].to(device).contiguous(), energy[:W].to(device).contiguous(), metadata, dt, box)
    return sh


# ----------------------------------------------------------------------------
# multi-step training over spatial shards (training.unrolled_loss over the ranks of a group)
# ----------------------------------------------------------------------------
#
# Frames are replicated: every rank holds the W true frames and every predicted frame of all N particles, and keeps
# activations only for the rows it owns.  A predicted frame is made from rows that each rank integrated (one all-gather,
# cgnn_frame_unpack) and is later read by other ranks' rows: a particle that changed tile, and under
# message_source="edge" every ghost sender's position.  The transpose of that all-gather is the sum over the ranks of
# every rank's gradient of the frame (:func:`reduce_frame_gradient`), of which each rank takes the rows it integrated.
#
# Every rank issues the same collectives in the same order whatever it owns: the links below never skip on a row count
# or on a missing gradient (the publish link materialises zeros), and every rank builds the same autograd structure.

class _LocalHalo:
    """The halo of a world of one without a process group: a tile that is the whole box has no ghosts."""

    def start(self, table: torch.Tensor):
        return None

    def finish(self, handle) -> None:
        pass

    def __call__(self, table: torch.Tensor) -> None:
        pass

    def start_return(self, grad_ghost: torch.Tensor):
        return grad_ghost.new_empty((0, grad_ghost.shape[1]))

    def finish_return(self, handle) -> torch.Tensor:
        return handle


def reduce_frame_gradient(grad: torch.Tensor, group=None) -> torch.Tensor:
    """The transpose of a predicted frame's all-gather: ``grad [N, 4]`` (three position components and the temperature of
    every particle: this rank's contributions to the gradient of one predicted frame) summed over the ranks, in place,
    by one all-reduce of ``16 N`` bytes.  Every rank then reads the rows it integrated (``ops.frame_grad_rows``)."""
    return _all_reduce_(grad, group)


class _PublishLink(torch.autograd.Function):
    """Rows a rank integrated -> the next frame of all particles.  Forward: the packed ``block [cap, ROLLOUT_ROW]`` of
    every rank gathered (one all-gather; a world of one keeps its block) and scattered by ``cgnn_frame_unpack`` into
    ``(pos [N, 3], temp [N])``.  ``new_pos [R, 3]`` / ``new_temp [R]`` are the block's differentiable rows (particles
    ``ids``).  Backward: the frame's gradient as ``[N, 4]``, zeros where no gradient arrived, summed over the ranks
    (:func:`reduce_frame_gradient`), read at ``ids`` (``cgnn_frame_grad_rows``)."""

    @staticmethod
    def forward(ctx, new_pos, new_temp, block, ids, n_total: int, group, gather: bool):
        rows = all_gather_rows(block, group) if gather else block
        dev = block.device
        # NaN until published: a particle no rank delivered cannot pass for a result
        pos = torch.full((n_total, 3), float("nan"), dtype=torch.float32, device=dev)
        temp = torch.full((n_total,), float("nan"), dtype=torch.float32, device=dev)
        ops.frame_unpack(rows, pos, temp)
        ctx.ids, ctx.n, ctx.group, ctx.dev = ids, int(n_total), group, dev
        ctx.set_materialize_grads(False)
        return pos, temp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_pos, d_temp):
        n, dev = ctx.n, ctx.dev
        grad = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        if d_pos is not None:
            grad[:, :3] = d_pos
        if d_temp is not None:
            grad[:, 3] = d_temp.reshape(n)
        grad = reduce_frame_gradient(grad, ctx.group)
        d_new_pos, d_new_temp = ops.frame_grad_rows(grad, ctx.ids)
        return d_new_pos, d_new_temp, None, None, None, None, None


def publish_frame(new_pos: torch.Tensor, new_temp: torch.Tensor, ids: torch.Tensor, n_total: int, cap: int, group=None,
                  block: Optional[torch.Tensor] = None):
    """The publish link on its own: the rows ``new_pos [R, 3]`` / ``new_temp [R]`` of the particles ``ids`` a rank
    integrated -> ``(pos [N, 3], temp [N])`` of all particles on every rank, differentiable in the rows.  ``cap``: the
    common block size (at least every rank's row count); ``block``: the packed rows when ``cgnn_rollout_integrate``
    made them already (``training._IntegrateLink``), else they are packed here."""
    r = ids.numel()
    if block is None:
        block = torch.zeros((int(cap), _lib.ROLLOUT_ROW), dtype=torch.float32, device=new_pos.device)
        block.view(torch.int32)[:, _lib.ROLLOUT_ROW - 1] = -1
        block[:r, :3] = new_pos.detach()
        block[:r, 3] = new_temp.detach().reshape(r)
        block.view(torch.int32)[:r, _lib.ROLLOUT_ROW - 1] = ids.to(torch.int32)
    return _PublishLink.apply(new_pos, new_temp, block, ids, int(n_total), group, _group_up())


def shard_record_bytes(n_owned: int, n_ghost: int, num_particles: int, num_neighbors: int) -> int:
    """What one rank of ``sharded_unrolled_loss(checkpoint="steps")`` keeps of one step until the backward, the small
    record: the replicated frame the step made (``16 N`` bytes) and the step's :class:`Shard` -- per edge its local
    sender and receiver rows and its features (``24 k n_owned``), the global ids of the owned and ghost rows and the send
    plan (``8 n_owned + 12 n_ghost``; the send plan counted at the ghost count).  The shard's whole-box maps (owner, global
    -> local) are dropped once the step's send plan and capacity are known."""
    n, g = int(n_owned), int(n_ghost)
    return 16 * int(num_particles) + 24 * n * int(num_neighbors) + 8 * n + 12 * g


def sharded_unrolled_training_bytes(n_owned: int, n_ghost: int, num_particles: int, num_neighbors: int, window: int,
                                    latent: int, hidden: int, num_hidden_layers: int, rounds: int, steps: int,
                                    edge_messages: bool = False, checkpoint: str = "none") -> int:
    """Device memory one rank of :func:`sharded_unrolled_loss` keeps alive until the backward: S times the shard's
    one-step activations (``training.unrolled_training_bytes`` over the ``n_owned`` rows and their ``n_owned k`` edges;
    under ``message_source="edge"`` also every round's input edge latents and local node table with its ghost rows,
    :func:`shard_edge_training_bytes`), one backward scratch, and the replicated frames: the W true and S predicted
    frames of all N particles, 16 bytes per particle and frame.  ``checkpoint="steps"``: one step's activations, the
    scratch, the W true frames and S small records (:func:`shard_record_bytes`, which holds a step's predicted frame)."""
    training.check_checkpoint(checkpoint, "sharded_unrolled_training_bytes")
    n, S = int(n_owned), int(steps)
    per_step, scratch = training._activation_floats(n, n * int(num_neighbors), window, latent, hidden, num_hidden_layers,
                                                    rounds, edge_messages)
    if edge_messages:       # the local node table of every round, with its ghost rows, and the ghosts' positions
        per_step += rounds * (n + int(n_ghost)) * latent + 3 * int(n_ghost)
    if checkpoint == "steps":
        return 4 * (per_step + scratch + int(window) * int(num_particles) * 4) + \
            S * shard_record_bytes(n, n_ghost, num_particles, num_neighbors)
    frames = (int(window) + S) * int(num_particles) * 4
    return 4 * (S * per_step + scratch + frames)


class _ShardedUnroll(training._Unroll):
    """``training._Unroll`` on one rank of :func:`sharded_unrolled_loss`: the same loop and checkpoint Function, with the
    step over the rows of a rank.  :meth:`plan` builds the step's shard; ``step`` then samples and integrates the owned
    rows (:meth:`_rows`) around :meth:`_predict` -- the sample of the ghost rows, :class:`ShardedTraining` with its halo
    exchanges, :func:`sharded_training_loss` with its all-reduces -- in each of its four uses (the plain step, the first
    run of a checkpointed step, its recomputation on the kept shard, the last step); :meth:`publish` gathers the rows
    into the next frame.  Whatever a rank holds, a step issues the same collectives in the same order: a rank that owns
    nothing runs it on empty blocks.  ``sample0(rows, want, targets=True)`` samples rows of the true window with step 0's
    noise."""

    def __init__(self, model, cfg, w: int, n: int, k: int, loss_weights, checkpoint: str, sample0, group, knn_grid: str,
                 min_image: bool, decomposition: str):
        super().__init__(model, cfg, w, n, k, loss_weights, checkpoint, sample0, knn_grid, min_image)
        self.group, self.decomposition, self.distributed = group, decomposition, _group_up()
        self.world, self.rank = _world_of(group)

    def plan(self, rec, pos_frames, tmp_frames, steps: int) -> None:
        """The step's :class:`Shard` and send capacity into ``rec``, from the wrapped last frame of all particles; before
        step 0 runs, the memory guard, agreed by all ranks."""
        cfg, model, s = self.cfg, self.model, rec.s
        with torch.no_grad():
            if s == 0:
                recent_all = self.sample0(None, ("recent_pos",), targets=False)["recent_pos"]
            else:
                recent_all = ops.training_sample(torch.stack([f.detach() for f in pos_frames[-2:]]),
                                                 torch.stack([f.detach() for f in tmp_frames[-2:]]), cfg.meta, cfg.dt,
                                                 cfg.box, 0.0, 0, 0, want=("recent_pos",), stats=cfg.stats)["recent_pos"]
            if not bool(torch.isfinite(recent_all).all()):        # the neighbour search must never see a NaN position
                raise CgnnError(f"sharded_unrolled_loss: the frame before step {s} holds non-finite positions (rows that "
                                f"were never published, or a diverged model)")
            sh = build_shard(recent_all, cfg.box, self.k, self.world, self.rank, decomposition=self.decomposition,
                             knn_grid=self.knn_grid, min_image_edge_attr=self.min_image, row_order="spatial")
            sh = exchange_requests(sh, self.group) if self.distributed else finish_shard(sh, sh.want_global)
            rec.shard, rec.cap = sh, _step_capacity(sh, self.world)[1]
        sh._g2l = sh._owner = None      # the whole-box maps have served (send plan, capacity): not part of the record
        if s == 0:      # one all-reduce (max) of a flag
            need = sharded_unrolled_training_bytes(sh.n_owned, sh.n_ghost, self.n, self.k, self.w, model._latent_size,
                                                   model._mlp_hidden_size, model._mlp_num_hidden_layers,
                                                   len(model.processor), steps, self.edge, self.checkpoint)
            free = training.free_device_bytes(recent_all.device)
            flag = _all_reduce_max_(torch.tensor([1.0 if need > free else 0.0], device=recent_all.device), self.group)
            if float(flag[0]) > 0.0:
                raise CgnnError(f"sharded_unrolled_loss: a rank lacks device memory for the activations of {steps} steps "
                                f"under checkpoint={self.checkpoint!r} (rank {self.rank}: about {need / 2**30:.2f} GiB for {sh.n_owned} owned and {sh.n_ghost} ghost "
                                f"rows of {self.n} particles, {self.k} neighbours, latent {model._latent_size}, "
                                f"{len(model.processor)} rounds; {free / 2**30:.2f} GiB are free)")

    def _rows(self, rec):
        return rec.shard.owned_global

    def _predict(self, rec, x, recent, y_acc, y_tr, frames, kept: bool):
        """On ``rec.shard``, kept or not: -> (acceleration, temp_rate, this rank's loss term) of the owned rows; fills
        ``rec.value`` and ``rec.terms`` (the global figures)."""
        cfg, sh = self.cfg, rec.shard
        runner = ShardedTraining(self.model, sh, None if self.distributed else _LocalHalo(), self.group)
        if self.edge:       # the shard's edge features as a function of the local rows [owned | ghosts]
            if rec.s == 0:
                recent_g = self.sample0(sh.ghost_global, ("recent_pos",), targets=False)["recent_pos"]
            else:
                recent_g, = training._SampleLink.apply(cfg, sh.ghost_global, ("recent_pos",), None, None, *frames)
            edge_attr = training._EdgeAttrLink.apply(torch.cat([recent, recent_g]), sh.edge_attr, sh.src_local, self.k,
                                                     sh.n_owned, lambda runner=runner: runner._csr)
            pred = runner(x, edge_attr)
        else:
            pred = runner(x)
        loss_s, rec.value, terms = sharded_training_loss(pred, y_acc, y_tr.reshape(-1, 1), self.n, cfg.dt,
                                                         *self.loss_weights, self.group, terms=True)
        rec.terms = terms.to(torch.float32)
        return pred["acceleration"], pred["temp_rate"], loss_s

    def publish(self, rec, rows_p, rows_t, block):
        """One all-gather of the ranks' blocks into the next frame of all particles, outside the checkpoint Function: the
        frame is gathered once, and its backward hands the step the gradient of the rows it integrated."""
        link = (rows_p, rows_t, block, rec.shard.owned_global, self.n, self.group, self.distributed)
        if rec.live:
            return _PublishLink.apply(*link)
        with torch.no_grad():
            return _PublishLink.apply(*link)


def sharded_unrolled_loss(model, position_seq: torch.Tensor, temperature_seq: torch.Tensor,
                          target_positions: torch.Tensor, target_temperatures: torch.Tensor, metadata: dict, *, dt: float,
                          box_size: float, num_neighbors: int = 16, noise_std: float = 0.0,
                          noise_seed: Optional[int] = None, noise_draw: int = 0, acc_loss_weight: float = 1.0,
                          temp_rate_loss_weight: float = 1.0, momentum_loss_weight: float = 0.0,
                          step_weights: Optional[Sequence[float]] = None, backprop_steps: Optional[int] = None,
                          min_image_edge_attr: bool = False, knn_grid: str = "uniform", decomposition: str = "uniform",
                          group=None, device=None, checkpoint: str = "none", density_loss_weight: float = 0.0,
                          density_mesh: Optional[int] = None, density_order: int = 2,
                          density_smoothing: float = 0.0, thermal_loss_weight: float = 0.0) -> "training.UnrolledLoss":
    """``training.unrolled_loss`` over the ranks of ``group`` (a world of one when no process group is up): the same
    arguments and meaning, S model steps unrolled from one window and differentiated through the whole chain, each rank
    computing the rows of its spatial tile.  Every rank passes the same windows and targets of all N particles (checked
    once, by one all-reduce of a checksum).  ``message_source="x_j"``, or ``"edge"`` with ``model.train_edge_messages``;
    ``train_precision`` "fp32" / "fp32x3"; one graph per call.

    Frames are replicated (``(W + S) N 16`` bytes per rank); activations are kept for the owned rows only
    (:func:`sharded_unrolled_training_bytes`; the ranks agree on the memory guard by one all-reduce after step 0's shard is
    known, and raise ``CgnnError`` together).  Step s on a rank: the wrapped last frame of all particles (detached) ->
    :func:`build_shard` (``row_order="spatial"``, so two calls give the same bits) and the ghost-id exchange, ownership
    following the particles from step to step; the sample of the owned rows (step 0 with the counter-based noise, later
    windows read the noisy frames, later targets are shifted by the last frame's noise); under ``"edge"`` the ghost
    rows' wrapped positions, the shard's edge features being a differentiable function of the local rows;
    :class:`ShardedTraining`; :func:`sharded_training_loss`; the integration of the owned rows; one all-gather into the
    next frame.  In the backward one all-reduce per live link sums the ranks' gradients of a predicted frame
    (:func:`reduce_frame_gradient`).

    Returns a ``training.UnrolledLoss``: ``loss`` is this rank's part to call ``.backward()`` on (afterwards every
    parameter's ``.grad`` is the global gradient on every rank), ``value`` the all-reduced global loss (0-d float64),
    ``step_losses [S, 3]`` the global terms, ``frames`` the whole predicted frames, ``graphs`` ``None``.
    ``noise_seed=None`` with noise in a world above one raises ``ValueError`` (``torch.initial_seed()`` differs between
    ranks).

    ``checkpoint="steps"``: ``training.unrolled_loss``'s activation checkpointing across steps, with the same meaning.
    Steps 0 .. S - 2 run without autograd; per step a rank keeps the :class:`Shard` (with the edge features its search
    made), the send capacity and the frames (:func:`shard_record_bytes`), so the backward neither searches nor
    synchronises with the host to build a shard.  The recomputation of a step runs :class:`ShardedTraining` with its
    halo exchanges, :func:`sharded_training_loss` with its all-reduces, the sample links and the integration of the
    owned rows again; the published frame is known and is not gathered again, its backward stays where it is.  Every
    rank issues the same collectives in the same order whatever it holds: a rank that owns nothing recomputes with empty
    blocks.  Frames, ``value`` and ``step_losses`` are those of ``"none"`` bit for bit.

    The density term of ``training.unrolled_loss`` is not computed over shards (a rank deposits its own rows, and
    meshes are not summed across ranks): the ``density_*`` arguments are named so that the two signatures stay one,
    and a non-zero ``density_loss_weight`` raises ``NotImplementedError`` before any device work.  The thermal term
    likewise: ``thermal_loss_weight`` is named, and refused when it is not zero."""
    w, n, S, weights = training._unroll_arguments(model, position_seq, temperature_seq, target_positions,
                                                  target_temperatures, step_weights, backprop_steps, num_neighbors,
                                                  knn_grid, min_image_edge_attr, checkpoint)
    if training._density_arguments(density_loss_weight, density_mesh, density_order, density_smoothing,
                                   "sharded_unrolled_loss") is not None:
        raise NotImplementedError("sharded_unrolled_loss: the density term is one box on one GPU (training.unrolled_loss); "
                                  "meshes are not summed across spatial shards")
    if training._density_arguments(thermal_loss_weight, density_mesh, density_order, density_smoothing,
                                   "sharded_unrolled_loss", name="thermal_loss_weight") is not None:
        raise NotImplementedError("sharded_unrolled_loss: the thermal term is one box on one GPU (training.unrolled_loss); "
                                  "meshes are not summed across spatial shards")
    if decomposition not in DECOMPOSITIONS:
        raise ValueError(f"sharded_unrolled_loss: decomposition {decomposition!r}; known: {DECOMPOSITIONS}")
    world, _ = _world_of(group)
    noisy = float(noise_std) != 0.0
    if noisy and noise_seed is None and world > 1:
        raise ValueError("sharded_unrolled_loss: noise needs an explicit noise_seed in a world above one "
                         "(torch.initial_seed() differs between ranks)")
    device = training._device_of(position_seq, device)
    if _group_up():
        tmp_in, tgt_t_in = temperature_seq.reshape(w, n), target_temperatures.reshape(S, n)
        check_same_data(torch.cat([position_seq, target_positions.to(position_seq.device)]),
                        torch.cat([tmp_in, tgt_t_in.to(tmp_in.device)]), device, group)
    cfg = training._LinkConfig(metadata, dt, box_size, n, device)
    pos_w, tmp_w, tgt_p, tgt_t = training._device_window(position_seq, temperature_seq, target_positions,
                                                         target_temperatures, device)
    sample0 = training._step0_sampler(cfg, pos_w, tmp_w, tgt_p[0], tgt_t[0], noise_std, noise_seed, noise_draw)
    unroll = _ShardedUnroll(model, cfg, w, n, int(num_neighbors), (acc_loss_weight, temp_rate_loss_weight,
                            momentum_loss_weight), checkpoint, sample0, group, knn_grid, min_image_edge_attr, decomposition)
    # the noise is replicated, like the frames, and not kept beyond the window
    window = training._noisy_window(pos_w, tmp_w, tgt_p, tgt_t,
                                    sample0(None, ("pos_noise", "temp_noise"), targets=False) if noisy else None)
    return unroll.run(*window, weights, backprop_steps)
