"""GPU: cgnn_balanced_planes and cgnn_tile_classify (csrc/decompose.hip) gated EXACTLY past one chunk of targets, past one trip
of the grid-stride loops and past one trip of the LDS count tables (tests/decompose_checks.py; the gates are tested on
themselves in tests/test_decompose_gates_cpu.py).  Every comparison is bit equality through an integer view, canaries included;
there are no tolerances.  The references sort every segment (any tile grid) and evaluate include/cgnn.h's float32 mask
expression in numpy.  Outputs and the workspace are pre-filled with canaries and handed to the C entries directly; the
positions lie between NaN rows.

Sizes: every family at every size of ``N_EDGES`` (at most 4097 rows) on every grid of ``GRIDS``, up to 16 x 16 x 16 and
4096 x 1 x 1; ``N_TWO_TRIPS`` = 2,098,180 rows (the first sizes at which a thread makes a second trip) on 2 x 2 x 2 and
4 x 4 x 4 only.  Left to tests/test_gpu_balanced_decomposition.py: real frames at worlds up to 8 and the sharded paths."""
import ctypes as C

import numpy as np
import pytest
import torch

import decompose_checks as dc
from cosmology_gnn_simulation_amd import _lib, dist as cdist, ops, synthetic
from migrate_checks import padded
from reduction_checks import PAD_ROWS

pytestmark = pytest.mark.gpu
DEV = "cuda"
WS_PAD = 4096                   # canary bytes on either side of the workspace
PLANE_PAD = 8                   # canary floats behind every planes buffer
MARGIN = 0.07                   # on computed planes: no dyadic number, the float32 expression decides


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _inner(full):
    v = full[PAD_ROWS:full.shape[0] - PAD_ROWS]
    assert v.is_contiguous()
    return v


def _sizes(grid):
    px, py, pz = grid
    return px - 1, px * (py - 1), px * py * (pz - 1)


def _planes(lib, pos, n, grid, want, with_owner, what, ws=None, null_single=False):
    """One call of cgnn_balanced_planes on canary-filled buffers, everything compared with ``want`` (planes_ref) and the
    canaries.  ``ws``: a workspace a former call left dirty.  ``null_single``: NULL for the planes of an axis with one part.
    -> (the planes on the device, the workspace)."""
    world = dc.world_of(grid)
    nbytes = lib.cgnn_balanced_planes_workspace_bytes(n, *grid)
    assert nbytes == dc.dec_layout(n, world)["total"], what
    edge0 = (np.arange(WS_PAD) % 251).astype(np.uint8)          # exactly the advertised size inside a larger buffer
    if ws is None:
        ws = (torch.arange(nbytes + 2 * WS_PAD, device=DEV) % 251).to(torch.uint8)
        ws[WS_PAD + nbytes:] = _dev(edge0)
    bufs0 = [dc.canary((s + PLANE_PAD,), 5000.0 + 100 * a) for a, s in enumerate(_sizes(grid))]
    bufs = [_dev(b) for b in bufs0]
    owner0 = dc.canary((n + PAD_ROWS,), 1 << 20, np.int32)
    owner = _dev(owner0)
    ptrs = [None if (null_single and grid[a] == 1) else bufs[a].data_ptr() for a in range(3)]
    assert lib.cgnn_balanced_planes(pos.data_ptr(), n, grid[0], grid[1], grid[2], ptrs[0], ptrs[1], ptrs[2],
                                    owner.data_ptr() if with_owner else None, ws.data_ptr() + WS_PAD, nbytes, _stream()) == 0, what
    for a, name in enumerate("xyz"):
        bufs0[a][:_sizes(grid)[a]] = want[a].reshape(-1)
        dc.assert_bits(bufs[a], bufs0[a], f"{what}: planes_{name} and canaries")
    if with_owner:
        owner0[:n] = want[3]
    dc.assert_bits(owner, owner0, f"{what}: owner and canaries")
    dc.assert_bits(ws[:WS_PAD], edge0, f"{what}: bytes before the workspace")
    dc.assert_bits(ws[WS_PAD + nbytes:], edge0, f"{what}: bytes behind the workspace")
    px, py, pz = grid
    s = _sizes(grid)
    return (bufs[0][:s[0]], bufs[1][:s[1]].view(px, py - 1), bufs[2][:s[2]].view(px, py, pz - 1)), ws


def _classify(lib, pos, n, grid, planes_d, rank, lo, hi, margin, box, want, what, outputs=(True, True, True)):
    """One call of cgnn_tile_classify with canaries behind each output; ``outputs``: which of (owner, counts, mask) are not
    NULL.  ``want``: (owner, counts, mask)."""
    world = dc.world_of(grid)
    firsts = (dc.canary((n + PAD_ROWS,), 1 << 20, np.int32), dc.canary((world + 8,), 1 << 40, np.int64),
              dc.canary((n + PAD_ROWS,), 100, np.uint8))
    devs = [_dev(f) for f in firsts]
    lo_c, hi_c = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
    ptrs = [d.data_ptr() if on else None for d, on in zip(devs, outputs)]
    cx, cy, cz = planes_d
    assert lib.cgnn_tile_classify(pos.data_ptr(), n, grid[0], grid[1], grid[2], cx.data_ptr(), cy.data_ptr(), cz.data_ptr(),
                                  rank, lo_c, hi_c, float(margin), float(box), ptrs[0], ptrs[1], ptrs[2], _stream()) == 0, what
    for first, dev, on, w, size, name in zip(firsts, devs, outputs, want, (n, world, n), ("owner", "counts", "mask")):
        if on:
            first[:size] = w
        dc.assert_bits(dev, first, f"{what}: {name} and canaries (outputs {outputs})")
    assert int(want[1].sum()) == n


# ---- cgnn_balanced_planes, and cgnn_tile_classify on its planes ----------------------------------------------------------------
def _planes_case(lib, name, n, grid, seed):
    world = dc.world_of(grid)
    pos = dc.frame(name, n, grid, seed)
    want = dc.planes_ref(pos, grid)
    full = _dev(padded(pos))
    pos_d = _inner(full)
    what = f"balanced_planes {name} n {n} grid {grid}"
    _planes(lib, pos_d, n, grid, want, False, what + " owner NULL", null_single=True)
    planes_d, ws = _planes(lib, pos_d, n, grid, want, True, what)
    _planes(lib, pos_d, n, grid, want, True, what + " again, on the workspace as the last call left it", ws=ws)
    counts = dc.counts_ref(want[3], world)
    for rank in dc.mask_ranks(world):
        lo, hi = dc.bounds_ref(want[:3], grid, rank, 1.0)
        mask = dc.mask_ref(pos, want[3], rank, lo, hi, MARGIN, 1.0)
        _classify(lib, pos_d, n, grid, planes_d, rank, lo, hi, MARGIN, 1.0, (want[3], counts, mask),
                  f"tile_classify on the planes of {name} n {n} grid {grid} rank {rank}")


@pytest.mark.parametrize("name", dc.FAMILIES)
@pytest.mark.parametrize("grid", dc.GRIDS, ids=dc.grid_id)
def test_planes_owner_counts_and_mask_at_every_edge(grid, name):
    """Every size of N_EDGES: the planes with owner == NULL (and NULL planes for an axis of one part), with an owner buffer,
    and again on the dirty workspace: planes, owner, the canaries behind them and around the workspace, bit for bit; then
    cgnn_tile_classify on those planes: owner, counts and the mask of ranks 0, the middle one and world - 1."""
    lib = _lib.load()
    for n in dc.N_EDGES:
        _planes_case(lib, name, n, grid, seed=n % 3)


@pytest.mark.parametrize("name", dc.FAMILIES)
@pytest.mark.parametrize("grid", dc.TWO_TRIP_GRIDS, ids=dc.grid_id)
def test_the_second_trip_of_the_grid_stride_loops(grid, name):
    """2,098,180 rows: 2048 workgroups, and the threads 0 .. 1027 make a second trip, a partial one."""
    n = dc.N_TWO_TRIPS
    assert dc.blocks(n) == dc.MAX_BLOCKS and dc.trips(n) == 2 and n - dc.FIRST_N_WITH_TWO_TRIPS + 1 == 1028
    lib = _lib.load()
    world = dc.world_of(grid)
    pos = dc.frame(name, n, grid)
    want = dc.planes_ref(pos, grid)
    pos_d = _inner(_dev(padded(pos)))
    what = f"balanced_planes {name} n {n} grid {grid}"
    _planes(lib, pos_d, n, grid, want, False, what + " owner NULL")
    planes_d, _ = _planes(lib, pos_d, n, grid, want, True, what)
    rank = world // 2
    lo, hi = dc.bounds_ref(want[:3], grid, rank, 1.0)
    _classify(lib, pos_d, n, grid, planes_d, rank, lo, hi, MARGIN, 1.0,
              (want[3], dc.counts_ref(want[3], world), dc.mask_ref(pos, want[3], rank, lo, hi, MARGIN, 1.0)),
              f"tile_classify {name} n {n} grid {grid}")


# ---- cgnn_tile_classify on hand-made planes --------------------------------------------------------------------------------------
def _hand_made(lib, grid, n, box, rank, margin, null_outputs=False):
    p = dc.mask_problem(1000 * n + rank, n, grid, box, rank, margin)
    planes_d = [_dev(c) for c in p["planes"]]                   # an axis of one part: no planes, a NULL pointer
    pos_d = _inner(_dev(padded(p["pos"])))
    want = (p["want_owner"], p["want_counts"], p["want_mask"])
    what = f"tile_classify grid {grid} n {n} box {box} rank {rank} margin {margin}"
    _classify(lib, pos_d, n, grid, planes_d, rank, p["lo"], p["hi"], p["margin"], box, want, what)
    for k in range(7 if null_outputs else 0):
        _classify(lib, pos_d, n, grid, planes_d, rank, p["lo"], p["hi"], p["margin"], box, want, what,
                  outputs=(bool(k & 1), bool(k & 2), bool(k & 4)))


@pytest.mark.parametrize("n", dc.N_EDGES)
@pytest.mark.parametrize("grid", dc.GRIDS, ids=dc.grid_id)
def test_tile_classify_on_hand_made_planes_and_planted_rows(grid, n):
    """Planes at multiples of box 2^-13 with duplicates (empty parts); rows exactly a reach from the centre, one exact step
    and one float32 neighbour on either side, rows on a plane value of their own column and its neighbours; margins 0,
    box / 32, one that covers every axis, one with width + 2 margin == box exactly (the axis is skipped) and box 2^-20 below
    it (tested).  Every margin and rank at 257, 1025 and 4097 rows, one margin in turn at the other sizes; every combination
    of NULL outputs at 1025 rows."""
    lib = _lib.load()
    i = dc.N_EDGES.index(n)
    for rank in dc.mask_ranks(dc.world_of(grid)):
        for margin in (dc.MARGINS if n in (257, 1025, 4097) else (dc.MARGINS[(i + rank) % len(dc.MARGINS)],)):
            _hand_made(lib, grid, n, (1.0, 2.0)[i % 2], rank, margin, null_outputs=n == 1025 and margin == "thirtysecond")


@pytest.mark.parametrize("grid", dc.TWO_TRIP_GRIDS, ids=dc.grid_id)
def test_tile_classify_on_hand_made_planes_makes_a_second_trip(grid):
    _hand_made(_lib.load(), grid, dc.N_TWO_TRIPS, 2.0, dc.world_of(grid) // 2, "thirtysecond")


# ---- the public path beyond a world of 8 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", (16, 27, 64))
def test_public_path_at_larger_worlds(world):
    """dist.balanced_planes, dist.owner_of and tile_bounds on the device against the CPU restatement, bit for bit, on a
    clustered frame of 20,000 particles."""
    n = 20_000
    cpu = synthetic.make_clustered_positions(n, seed=5)
    pos = cpu.to(DEV)
    grid = cdist.tile_grid(world)
    want = cdist.balanced_planes(cpu, 1.0, world)
    want_owner = cdist.owner_of(cpu, 1.0, world, want)
    ref = dc.planes_ref(cpu.numpy(), grid)
    got = cdist.balanced_planes(pos, 1.0, world)
    assert got.grid == grid and all(g.is_cuda for g in got.tensors())
    for g, w, r in zip(got.tensors(), want.tensors(), ref[:3]):
        dc.assert_bits(g, w, f"dist.balanced_planes world {world}")
        dc.assert_bits(w, r, f"the two references, world {world}")
    dc.assert_bits(cdist.owner_of(pos, 1.0, world, got), want_owner, f"dist.owner_of world {world}")
    dc.assert_bits(want_owner, ref[3], "the two references' owners")
    for rank in range(world):
        assert cdist.tile_bounds(1.0, world, rank, got) == cdist.tile_bounds(1.0, world, rank, want) == \
            tuple(dc.bounds_ref(ref[:3], grid, rank, 1.0)), (world, rank)
    counts = torch.bincount(want_owner.long(), minlength=world)
    assert int(counts.max()) <= 1.01 * n / world


@pytest.fixture(scope="module")
def frame27():
    """The frame, the global search and the CPU restatement's owners, made once for the cases below."""
    n, k, world = 20_000, 16, 27
    cpu = synthetic.make_clustered_positions(n, seed=5)
    pos = cpu.to(DEV)
    senders, _, _ = ops.knn_periodic(pos, 1.0, k, want_edge_attr=False)
    want_owner = cdist.owner_of(cpu, 1.0, world, cdist.balanced_planes(cpu, 1.0, world))
    n_uniform = torch.bincount(cdist.owner_of(pos, 1.0, world).long(), minlength=world)
    return n, k, world, cpu, pos, senders.view(n, k).long(), want_owner, n_uniform


@pytest.mark.parametrize("first", range(0, 27, 3))
def test_device_shards_of_27_ranks_equal_the_cpu_restatement_and_the_global_search(frame27, first):
    """test_gpu_balanced_decomposition.py::test_device_shards_equal_the_cpu_restatement_and_the_global_search at a world of
    27, three ranks per case: its assertions, with two restated.  The ranks of one case cannot be concatenated to all
    particles, so every rank's owned ids are held to the CPU owner's (which partitions them).  And its bound on what equal
    volumes give this frame, (0.4 + 0.5 world) / world n, is written for grids whose first tile is the whole octant of the
    halo (worlds 2, 4, 8); the 3 x 3 x 3 grid cuts the halo, the CPU expression gives 9035 of 20,000 in its fullest tile,
    twelve times the mean: the device counts are held to that expression."""
    n, k, world, cpu, pos, want, want_owner, n_uniform = frame27
    ranks = range(first, first + 3)
    shards = [cdist.build_shard(pos, 1.0, k, world, r, decomposition="balanced") for r in ranks]
    for r, sh in zip(ranks, shards):
        assert torch.equal(sh._owner.cpu(), want_owner)
        assert sh._counts.tolist() == torch.bincount(want_owner.long(), minlength=world).tolist()
        assert sh.n_owned == sh._counts[r]
        table = torch.cat([sh.owned_global, sh.ghost_global])
        assert torch.equal(table[sh.src_local.long()].view(sh.n_owned, k), want[sh.owned_global]), (world, r)
        assert torch.equal(torch.sort(sh.owned_global).values.cpu(), torch.nonzero(want_owner == r).squeeze(1))
    assert max(sh.n_owned for sh in shards) <= 1.01 * n / world
    assert n_uniform.tolist() == torch.bincount(cdist.owner_of(cpu, 1.0, world).long(), minlength=world).tolist()
    assert int(n_uniform.max()) >= 12 * n / world


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------
def test_the_ops_wrappers_on_a_straddling_grid():
    grid, n = (4, 4, 4), 4097
    pos = dc.frame("ties_across_rank", n, grid, seed=2)
    want = dc.planes_ref(pos, grid)
    pos_d = _dev(pos)
    cx, cy, cz, owner = ops.balanced_planes(pos_d, grid, want_owner=True)
    for g, w in zip((cx, cy, cz, owner), want):
        assert g.shape == w.shape
        dc.assert_bits(g, w, "ops.balanced_planes")
    assert ops.balanced_planes(pos_d, grid)[3] is None
    rank = 37
    lo, hi = dc.bounds_ref(want[:3], grid, rank, 1.0)
    got = ops.tile_classify(pos_d, (cx, cy, cz), rank, lo, hi, MARGIN, 1.0)
    dc.assert_bits(got[0], want[3], "ops.tile_classify owner")
    dc.assert_bits(got[1], dc.counts_ref(want[3], 64), "ops.tile_classify counts")
    assert got[2].dtype == torch.bool
    dc.assert_bits(got[2].view(torch.uint8), dc.mask_ref(pos, want[3], rank, lo, hi, MARGIN, 1.0), "ops.tile_classify mask")
