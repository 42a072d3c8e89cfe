"""CPU: the balanced decomposition of cosmology_gnn_simulation_amd/dist.py (tiles cut at particle-count quantiles).

The definition is restated here by brute force (numpy sort per segment) and the package's torch restatement is held to
it; the sharding plan over balanced tiles is held to the global oracle search, as tests/test_dist_cpu.py holds the
equal-volume one."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cosmology_gnn_simulation_amd import dist as cdist
from cosmology_gnn_simulation_amd import synthetic
from oracle import cpu_ref

BOX = 1.0
WORLDS = (1, 2, 3, 4, 6, 8)


# ----------------------------------------------------------------------------
# the definition, read literally
# ----------------------------------------------------------------------------

def _cut(v: np.ndarray, p: int) -> np.ndarray:
    """Part of every element of the segment ``v`` on an axis with ``p`` parts: planes c_j = s[(j m) // p], part =
    #{ j : c_j <= v }."""
    m = v.shape[0]
    part = np.zeros(m, dtype=np.int64)
    if m == 0:
        return part
    s = np.sort(v)
    for j in range(1, p):
        part += (s[(j * m) // p] <= v)
    return part


def brute_force_owner(pos: torch.Tensor, world: int) -> np.ndarray:
    px, py, pz = cdist.tile_grid(world)
    x = pos.numpy().astype(np.float32)
    n = x.shape[0]
    ix = _cut(x[:, 0], px)
    iy = np.zeros(n, dtype=np.int64)
    iz = np.zeros(n, dtype=np.int64)
    for i in range(px):
        slab = np.nonzero(ix == i)[0]
        iy[slab] = _cut(x[slab, 1], py)
        for j in range(py):
            col = slab[iy[slab] == j]
            iz[col] = _cut(x[col, 2], pz)
    return (ix * py + iy) * pz + iz


def _frames():
    g = torch.Generator().manual_seed(11)
    lattice = torch.stack(torch.meshgrid(*[torch.arange(16, dtype=torch.float32) / 16] * 3, indexing="ij"),
                          dim=-1).reshape(-1, 3)
    lattice = lattice[torch.randperm(lattice.shape[0], generator=g)].contiguous()
    outside = torch.rand(5000, 3, generator=g) * BOX
    outside[::7] -= 1.25          # some coordinates below 0 ...
    outside[3::11] += 1.5         # ... and some at or above the box
    return {"clustered": synthetic.make_clustered_positions(20_000),
            "uniform": torch.rand(20_000, 3, generator=g) * BOX,
            "lattice": lattice,
            "outside": outside}


@pytest.mark.parametrize("world", WORLDS)
def test_torch_restatement_equals_the_brute_force_definition(world):
    for name, pos in _frames().items():
        want = brute_force_owner(pos, world)
        planes = cdist.balanced_planes(pos, BOX, world)
        assert planes.grid == cdist.tile_grid(world)
        got = cdist.owner_of(pos, BOX, world, planes)
        assert got.dtype == torch.int32
        assert np.array_equal(got.numpy().astype(np.int64), want), (name, world)


# the 16^3 lattice has 256 particles on every plane value: "a particle on a plane goes to the upper part" decides.
# Counts per rank as the brute-force reading of the definition gives them (derived by hand below, pinned here):
#   an axis with 16 distinct values, 16 m' each: p = 2 -> plane s[m/2] = the 9th value -> 8 + 8 values;
#   p = 3 -> planes s[m/3], s[2m/3] = the 6th and 11th values -> 5 + 5 + 6 values.
LATTICE_COUNTS = {
    1: [4096],
    2: [2048, 2048],
    3: [1280, 1280, 1536],
    4: [1024] * 4,
    6: [640, 640, 640, 640, 768, 768],
    8: [512] * 8,
}


@pytest.mark.parametrize("world", WORLDS)
def test_lattice_ties_give_the_pinned_counts(world):
    pos = _frames()["lattice"]
    want = np.bincount(brute_force_owner(pos, world), minlength=world).tolist()
    assert want == LATTICE_COUNTS[world]
    got = cdist.owner_of(pos, BOX, world, cdist.balanced_planes(pos, BOX, world))
    assert torch.bincount(got.long(), minlength=world).tolist() == want


def test_coincident_particles_leave_empty_tiles_that_work():
    """All particles on one point: every plane equals that point, every particle goes to the last tile."""
    pos = torch.full((64, 3), 0.375)
    for world in (2, 4, 8):
        planes = cdist.balanced_planes(pos, BOX, world)
        own = cdist.owner_of(pos, BOX, world, planes)
        assert own.tolist() == [world - 1] * 64
        assert np.array_equal(brute_force_owner(pos, world), own.numpy())
    shards = [cdist.build_shard(pos, BOX, 4, 2, r, knn_fn=_oracle_knn,
                                decomposition="balanced") for r in range(2)]
    assert [sh.n_owned for sh in shards] == [0, 64] and shards[0].n_ghost == 0


@pytest.mark.parametrize("world,uniform_factor", [(2, 1.4), (4, 2.4), (8, 4.4)])
def test_balance_of_the_definition_on_the_clustered_frame(world, uniform_factor):
    """A condition on the definition (the brute force), not on the code under test: the fullest rank holds at most
    1.01 N / world particles, while equal-volume tiles give it (0.5 + 0.5 / world) N: 1.5 / 2.5 / 4.5 x the mean.

    Measured at N = 20,000 (make_clustered_positions defaults): balanced maxima 10000 / 5000 / 2500 for worlds 2 / 4
    / 8, i.e. 1.0000 x N / world each (no float32 plane ties); equal-volume maxima 14965 / 12471 / 11227, i.e. 1.497 /
    2.494 / 4.491 x N / world."""
    pos = synthetic.make_clustered_positions(20_000)
    n = pos.shape[0]
    balanced = np.bincount(brute_force_owner(pos, world), minlength=world)
    uniform = torch.bincount(cdist.owner_of(pos, BOX, world).long(), minlength=world)
    print(f"world {world}: balanced max {int(balanced.max())}, uniform max {int(uniform.max())}, mean {n / world}")
    assert balanced.sum() == n
    assert balanced.max() <= 1.01 * n / world
    assert int(uniform.max()) >= uniform_factor * n / world


@pytest.mark.parametrize("world", [2, 3, 4, 6, 8])
def test_tile_bounds_invert_owner_of_with_planes(world):
    g = torch.Generator().manual_seed(12)
    for pos in (synthetic.make_clustered_positions(3000, seed=3), torch.rand(3000, 3, generator=g) * BOX,
                _frames()["lattice"]):
        n = pos.shape[0]
        planes = cdist.balanced_planes(pos, BOX, world)
        own = cdist.owner_of(pos, BOX, world, planes)
        covered = torch.zeros(n, dtype=torch.int64)
        for r in range(world):
            lo, hi = cdist.tile_bounds(BOX, world, r, planes)
            inside = torch.ones(n, dtype=torch.bool)
            for a in range(3):
                inside &= (pos[:, a] >= lo[a]) & (pos[:, a] < hi[a])
            assert torch.equal(inside, own == r), (world, r)
            covered += inside
        assert bool((covered == 1).all())


def test_uniform_stays_the_default_and_keeps_its_bits():
    pos = synthetic.make_clustered_positions(2000, seed=4)
    assert torch.equal(cdist.owner_of(pos, BOX, 8), cdist.owner_of(pos, BOX, 8, None))
    assert cdist.tile_bounds(BOX, 8, 5) == cdist.tile_bounds(BOX, 8, 5, None) == ([0.5, 0.0, 0.5], [1.0, 0.5, 1.0])
    a = cdist.build_shard(pos, BOX, 8, 4, 1, knn_fn=_oracle_knn)
    b = cdist.build_shard(pos, BOX, 8, 4, 1, knn_fn=_oracle_knn, decomposition="uniform")
    assert a._planes is None and b._planes is None
    assert torch.equal(a.owned_global, b.owned_global) and torch.equal(a.src_local, b.src_local)
    assert torch.equal(a._owner, cdist.owner_of(pos, BOX, 4))
    with pytest.raises(ValueError):
        cdist.build_shard(pos, BOX, 8, 4, 1, knn_fn=_oracle_knn, decomposition="by-volume")


def test_clustered_generators_are_deterministic_and_in_the_box():
    a, b = synthetic.make_clustered_positions(5000), synthetic.make_clustered_positions(5000)
    assert torch.equal(a, b) and a.shape == (5000, 3) and a.dtype == torch.float32
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
    assert not torch.equal(a, synthetic.make_clustered_positions(5000, seed=1))
    in_octant = int(((a < 0.5).all(dim=1)).sum())
    assert 0.5 * 5000 <= in_octant <= 0.6 * 5000          # the halo, plus an eighth of the uniform half
    snap = synthetic.make_clustered_snapshot(1000, seed=9)
    ref = synthetic.make_snapshot(1000, seed=9)
    assert snap["Coordinates"].shape == ref["Coordinates"].shape
    assert snap["InternalEnergy"].shape == ref["InternalEnergy"].shape
    assert torch.equal(snap["Coordinates"][0], synthetic.make_clustered_positions(1000, seed=9))
    assert float(snap["Coordinates"].min()) >= 0.0 and float(snap["Coordinates"].max()) < 1.0


# ----------------------------------------------------------------------------
# the sharding plan over balanced tiles
# ----------------------------------------------------------------------------

N, K = 900, 8


def _oracle_knn(pos, box, k, query_ids):
    ei, ea = cpu_ref.knn_periodic(pos, box, k)
    q = query_ids.long()
    snd = ei[0].view(pos.shape[0], k)[q].reshape(-1).to(torch.int32)
    attr = ea.view(pos.shape[0], k, 4)[q].reshape(-1, 4)
    return snd, attr, None


def _small_clustered():
    return synthetic.make_clustered_positions(N, seed=21)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_balanced_shards_equal_the_global_search_and_partition_the_particles(world):
    pos = _small_clustered()
    ei, _ = cpu_ref.knn_periodic(pos, BOX, K)
    want = ei[0].view(N, K)
    shards = [cdist.build_shard(pos, BOX, K, world, r, knn_fn=_oracle_knn, decomposition="balanced")
              for r in range(world)]
    own = torch.from_numpy(brute_force_owner(pos, world))
    for r, sh in enumerate(shards):
        assert sh._planes is not None and torch.equal(sh._owner.long(), own)
        assert torch.equal(torch.sort(sh.owned_global).values, torch.nonzero(own == r).squeeze(1))
        local_to_global = torch.cat([sh.owned_global, sh.ghost_global])
        assert torch.equal(local_to_global[sh.src_local.long()].view(sh.n_owned, K), want[sh.owned_global]), (world, r)
    assert torch.equal(torch.sort(torch.cat([sh.owned_global for sh in shards])).values, torch.arange(N))
    assert max(sh.n_owned for sh in shards) <= -(-N // world) + 2       # nested ceil; no ties in this frame
    # ghost plans: every ghost is grouped under its owner, and the peers' requests resolve to owned rows
    for r, sh in enumerate(shards):
        cdist.finish_shard(sh, [shards[p].want_global[r] for p in range(world)])
        assert sh.send_counts[r] == 0
        got_owner = own[sh.ghost_global].tolist()
        assert got_owner == sorted(got_owner) and r not in got_owner
        assert torch.equal(sh.owned_global[sh.send_idx.long()],
                           torch.cat([shards[p].want_global[r] for p in range(world)]))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pos = _small_clustered()
        sh = cdist.build_shard(pos, BOX, K, world, rank, knn_fn=_oracle_knn, decomposition="balanced")
        sh = cdist.exchange_requests(sh)
        table_global = torch.arange(N, dtype=torch.float32).view(N, 1).repeat(1, 4) + \
            torch.tensor([0.0, 0.25, 0.5, 0.75])
        table = torch.zeros(sh.n_local, 4)
        table[:sh.n_owned] = table_global[sh.owned_global]
        halo = cdist.HaloExchange(sh, pack_fn=lambda t, idx, out: out.copy_(t[idx.long()]))
        halo(table)
        ok_ghost = torch.equal(table[sh.n_owned:], table_global[sh.ghost_global])
        ei, _ = cpu_ref.knn_periodic(pos, BOX, K)
        want = cpu_ref.propagate_add(table_global, ei)[sh.owned_global]
        got = table[sh.src_local.long()].view(sh.n_owned, K, 4).sum(dim=1)
        q.put((rank, sh.n_owned, sh.n_ghost, ok_ghost, bool(torch.allclose(got, want)), sum(sh.send_counts)))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(120)
def test_two_rank_halo_exchange_over_gloo_balanced():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=100) for _ in procs)
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert [r[1] for r in res] == [N // 2, N // 2]           # balanced: half of the particles each
    assert all(r[2] > 0 and r[3] and r[4] for r in res)     # ghosts exist, arrive intact, sums match
    assert res[0][5] == res[1][2] and res[1][5] == res[0][2]  # rows sent == rows the peer receives
