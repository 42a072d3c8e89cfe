"""CPU: the host logic of the sharded rollout with particle migration (dist.sharded_rollout(storage="owned"),
dist.MigratingRollout): refusals before any device work, the torch restatement of the halo peer test, the subset-space
numbering against build_shard, and the id search of the send plan.  The oracle k-NN stands in for the HIP search."""
import pytest
import torch

from cosmology_gnn_simulation_amd import dist as cdist, ops
from oracle import cpu_ref

N, K, BOX, W = 600, 8, 1.0, 6


def _oracle_knn(pos, box, k, query_ids):
    ei, ea = cpu_ref.knn_periodic(pos, box, k)
    q = query_ids.long()
    snd = ei[0].view(pos.shape[0], k)[q].reshape(-1).to(torch.int32)
    attr = ea.view(pos.shape[0], k, 4)[q].reshape(-1, 4)
    return snd, attr, None


def _positions(seed=77, n=N, clustered=False):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=g) * BOX
    if clustered:
        blob = torch.remainder(0.3 + 0.05 * torch.randn(n - n // 5, 3, generator=g), BOX)
        pos = torch.cat([blob, pos[:n // 5]])
    return pos


class _NoModel:
    """Stands where a model would: a refusal must come before anything asks it for a device or a parameter."""

    def parameters(self):
        raise AssertionError("device work was started")

    def eval(self):
        raise AssertionError("device work was started")


def _data(n=50, frames=W):
    g = torch.Generator().manual_seed(1)
    return {"Coordinates": torch.rand(frames, n, 3, generator=g), "InternalEnergy": torch.rand(frames, n, 1, generator=g)}


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_unknown_storage_is_refused_before_device_work():
    with pytest.raises(ValueError, match="storage"):
        cdist.sharded_rollout(_NoModel(), _data(), {}, 0.0, 0.01, BOX, W, 16, 2, storage="shared")
    assert cdist.ROLLOUT_STORAGE == ("replicated", "owned")


def test_rollout_arguments_cases_are_refused_in_owned_mode():
    data = _data()
    for kwargs in (dict(window_size=1), dict(num_neighbors=51), dict(num_steps=-1)):
        args = dict(window_size=W, num_neighbors=16, num_steps=2)
        args.update(kwargs)
        with pytest.raises(ValueError):
            cdist.sharded_rollout(_NoModel(), data, {}, 0.0, 0.01, BOX, storage="owned", **args)
    with pytest.raises(ValueError):
        cdist.sharded_rollout(_NoModel(), _data(frames=W - 1), {}, 0.0, 0.01, BOX, W, 16, 2, storage="owned")


def test_a_world_above_the_peer_mask_is_refused():
    assert cdist.MAX_MIGRATING_WORLD == 64
    with pytest.raises(ValueError, match="64"):
        cdist.check_rollout_storage("owned", 65)
    assert cdist.check_rollout_storage("owned", 64) == "owned"
    assert cdist.check_rollout_storage("replicated", 4096) == "replicated"
    ids = torch.arange(5)
    with pytest.raises(ValueError, match="64"):
        cdist.MigratingRollout(_NoModel(), ids, torch.zeros(W, 5, 3), torch.zeros(W, 5, 1), n_total=100, metadata={},
                               dt=0.01, box_size=BOX, window_size=W, num_neighbors=4, world=128, rank=0)


def test_migrating_rollout_refuses_bad_arguments_before_device_work():
    ids = torch.arange(5)
    ok = dict(n_total=100, metadata={}, dt=0.01, box_size=BOX, window_size=W, num_neighbors=4, world=2, rank=0)
    for bad in (dict(n_total=torch.zeros(100)), dict(n_total=10.5), dict(window_size=1), dict(window_size=33),
                dict(rank=2), dict(num_neighbors=101), dict(num_neighbors=0), dict(knn_grid="hexagonal"),
                dict(n_total=2 ** 31)):
        with pytest.raises(ValueError):
            cdist.MigratingRollout(_NoModel(), ids, torch.zeros(W, 5, 3), torch.zeros(W, 5, 1), **dict(ok, **bad))
    with pytest.raises(ValueError, match="window"):         # the window of 4 particles for 5 ids
        cdist.MigratingRollout(_NoModel(), ids, torch.zeros(W, 4, 3), torch.zeros(W, 4, 1), **ok)
    planes = cdist.balanced_planes(_positions(), BOX, 4)
    with pytest.raises(ValueError, match="planes"):         # planes of a world of 4 for a world of 2
        cdist.MigratingRollout(_NoModel(), ids, torch.zeros(W, 5, 3), torch.zeros(W, 5, 1), planes=planes, **ok)


# ---- the peer test -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("decomposition", ["uniform", "balanced"])
def test_peer_mask_marks_exactly_what_every_tile_searches(world, decomposition):
    """For every tile p: the rows the other ranks mark for p are exactly build_shard's search subset of p (_near_tile |
    owner == p) minus p's own rows.  The margins include one that covers an axis of the tile grid."""
    pos = _positions(seed=5, n=2000, clustered=decomposition == "balanced")
    planes = cdist.balanced_planes(pos, BOX, world) if decomposition == "balanced" else None
    owner = cdist.owner_of(pos, BOX, world, planes)
    covered = 0
    for margin in (0.03, 0.11, 0.26):
        marks = torch.zeros(pos.shape[0], world, dtype=torch.bool)
        for r in range(world):
            held = torch.nonzero(owner == r).squeeze(1)
            m = cdist.peer_mask(pos[held], BOX, world, r, margin, planes)
            assert m.shape == (held.numel(), world) and not bool(m[:, r].any())
            marks[held] = m
        for p in range(world):
            lo, hi = cdist.tile_bounds(BOX, world, p, planes)
            covered += sum(1 for a in range(3) if hi[a] - lo[a] + 2 * margin >= BOX and hi[a] - lo[a] < BOX)
            want = (cdist._near_tile(pos, BOX, lo, hi, margin) | (owner == p)) & (owner != p)
            assert torch.equal(marks[:, p], want), (world, decomposition, margin, p)
    assert covered > 0          # a split axis whose expanded tile wraps around the box was among the cases


def test_first_margin_is_build_shards():
    calls = []

    def knn(p, b, kk, q):
        calls.append(p.shape[0])
        return _oracle_knn(p, b, kk, q)
    pos = _positions(seed=6, n=3000)
    sh = cdist.build_shard(pos, BOX, K, 8, 3, knn_fn=knn)
    margin = cdist.first_margin(BOX, K, pos.shape[0])
    lo, hi = cdist.tile_bounds(BOX, 8, 3)
    near = cdist._near_tile(pos, BOX, lo, hi, margin) | (cdist.owner_of(pos, BOX, 8) == 3)
    assert sh.searches == 1 and sh.subset_rows == int(near.sum()) < pos.shape[0]


# ---- numbering in subset space -------------------------------------------------------------------------------------------

def _subset_inputs(pos, world, rank, planes):
    """What a rank of the migrating rollout has after its search, made the way build_shard selects: the search set in
    ascending id (held rows + what the peers mark for it), who holds each row, the owned queries and their senders."""
    owner = cdist.owner_of(pos, BOX, world, planes)
    margin = cdist.first_margin(BOX, K, pos.shape[0])
    lo, hi = cdist.tile_bounds(BOX, world, rank, planes)
    while True:
        near = cdist._near_tile(pos, BOX, lo, hi, margin) | (owner == rank)
        sub = torch.nonzero(near).squeeze(1)
        pos_sub, owner_sub = pos[sub].contiguous(), owner[sub]
        owned_s = torch.nonzero(owner_sub == rank).squeeze(1)
        senders_s, edge_attr, _ = _oracle_knn(pos_sub, BOX, K, owned_s)
        if sub.numel() == pos.shape[0] or owned_s.numel() == 0:
            break
        kth = senders_s.view(-1, K)[:, K - 1].long()
        d = torch.abs(pos_sub[kth] - pos_sub[owned_s])
        d = torch.minimum(d, BOX - d)
        if float(d.norm(dim=1).max()) <= margin:
            break
        margin *= 2.0
    return sub, owner_sub, owned_s, senders_s, edge_attr


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("decomposition", ["uniform", "balanced"])
def test_subset_shard_is_build_shards_shard(world, decomposition):
    pos = _positions(seed=11 + world, n=3000 if world == 8 else 900, clustered=decomposition == "balanced")
    planes = cdist.balanced_planes(pos, BOX, world) if decomposition == "balanced" else None
    shards = []
    subsets = 0
    for r in range(world):
        want = cdist.build_shard(pos, BOX, K, world, r, knn_fn=_oracle_knn, decomposition=decomposition)
        sub, owner_sub, owned_s, senders_s, edge_attr = _subset_inputs(pos, world, r, planes)
        subsets += sub.numel() < pos.shape[0]
        got = cdist.subset_shard(r, world, K, owned_s, senders_s, edge_attr, owner_sub.to(torch.int32), sub)
        for name in ("rank", "world", "k", "n_owned", "n_ghost", "n_interior", "recv_counts"):
            assert getattr(got, name) == getattr(want, name), (r, name)
        for name in ("owned_global", "ghost_global", "src_local", "dst_local", "edge_attr"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.dtype == b.dtype and torch.equal(a, b), (r, name)
        assert len(got.want_global) == world
        assert all(torch.equal(a, b) for a, b in zip(got.want_global, want.want_global))
        shards.append((got, want))
    if world == 8:
        assert subsets > 0       # real subsets, not only the whole box, went through the helper
    # the send plans: the search in the sorted held ids gives finish_shard's rows
    for r, (got, want) in enumerate(shards):
        requests = [shards[p][0].want_global[r] for p in range(world)]
        cdist.finish_shard_by_search(got, requests)
        cdist.finish_shard(want, requests)
        assert got.send_counts == want.send_counts and got.send_idx.dtype == want.send_idx.dtype
        assert torch.equal(got.send_idx, want.send_idx)


def test_subset_shard_of_the_whole_box_needs_no_ids():
    pos = _positions(seed=3, n=300)
    want = cdist.build_shard(pos, BOX, K, 2, 1, knn_fn=_oracle_knn)
    owner = cdist.owner_of(pos, BOX, 2)
    owned_s = torch.nonzero(owner == 1).squeeze(1)
    senders_s, edge_attr, _ = _oracle_knn(pos, BOX, K, owned_s)
    got = cdist.subset_shard(1, 2, K, owned_s, senders_s, edge_attr, owner)
    assert torch.equal(got.owned_global, want.owned_global) and torch.equal(got.src_local, want.src_local)
    assert torch.equal(got.ghost_global, want.ghost_global)


# ---- the send plan's id search -------------------------------------------------------------------------------------------

def test_send_plan_search_raises_on_an_id_that_is_not_held():
    held = torch.tensor([3, 8, 9, 40, 41])
    local = torch.tensor([4, 0, 2, 1, 3], dtype=torch.int32)
    got = cdist.held_rows_of(held, local, torch.tensor([40, 3, 9]), "rank 0: rank 1")
    assert got.tolist() == [1, 4, 2]
    assert cdist.held_rows_of(held, local, torch.tensor([], dtype=torch.int64), "x").numel() == 0
    for missing in ([7], [3, 42], [0], [41, 10, 8]):
        with pytest.raises(RuntimeError, match="does not own"):
            cdist.held_rows_of(held, local, torch.tensor(missing), "rank 0: rank 1")
    with pytest.raises(RuntimeError, match="does not own"):
        cdist.held_rows_of(held[:0], local[:0], torch.tensor([1]), "rank 0: rank 1")
    pos = _positions(seed=9, n=400)
    sub, owner_sub, owned_s, senders_s, edge_attr = _subset_inputs(pos, 2, 0, None)
    sh = cdist.subset_shard(0, 2, K, owned_s, senders_s, edge_attr, owner_sub.to(torch.int32), sub)
    theirs = torch.nonzero(cdist.owner_of(pos, BOX, 2) == 1).squeeze(1)[:3]
    with pytest.raises(RuntimeError, match="rank 1 requested rows this rank does not own"):
        cdist.finish_shard_by_search(sh, [sh.owned_global[:0], theirs])


def test_group_offsets_are_starts_plus_the_rows_of_earlier_blocks():
    counts = torch.tensor([[2, 0, 1], [0, 3, 1], [4, 0, 0]], dtype=torch.int32)
    starts = torch.tensor([0, 6, 9])
    got = ops.group_offsets(counts, starts)
    assert got.dtype == torch.int32 and got.tolist() == [[0, 6, 9], [2, 6, 10], [2, 9, 11]]
    assert ops.migrate_blocks(0) == 0 and ops.migrate_blocks(256) == 1 and ops.migrate_blocks(257) == 2
