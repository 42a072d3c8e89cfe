"""CPU: host logic of edge-mode training over spatial shards (dist.ShardedEdgeTraining) -- the interior split on a 32-edge
tile, the per-rank memory estimate, the TILED32 edge views and which runner ShardedTraining picks."""
import math

import pytest
import torch

from cosmology_gnn_simulation_amd import dist as cdist, graph_network, ops, training
from cosmology_gnn_simulation_amd._lib import CgnnError


@pytest.mark.parametrize("k", [1, 4, 5, 8, 12, 16, 24, 32, 48])
def test_edge_split_rows_aligns_to_a_tile_and_never_exceeds_the_interior(k):
    for ni in list(range(0, 70)) + [999, 1000, 1001, 108_622, 124_691]:
        ns = cdist.edge_split_rows(ni, k)
        assert 0 <= ns <= ni
        assert (ns * k) % 32 == 0
        step = 32 // math.gcd(k, 32)
        assert ni - ns < step                     # the largest aligned count: one more step would pass n_interior
    assert cdist.edge_split_rows(7, 12) == 0      # 12 rows are 384 edges: nothing below 8 receivers aligns
    assert cdist.edge_split_rows(100, 12) == 96
    assert cdist.edge_split_rows(100, 16) == 100
    assert cdist.edge_split_rows(101, 16) == 100
    assert cdist.edge_split_rows(33, 32) == 33
    with pytest.raises(ValueError):
        cdist.edge_split_rows(-1, 16)
    with pytest.raises(ValueError):
        cdist.edge_split_rows(10, 0)


def test_cfg4_fits_one_mi355x_per_rank_when_split_eight_ways():
    """cfg4: 4 M particles, k = 16, D = H = 128, 2 hidden layers, 10 rounds.  The unsharded estimate is above one
    MI355X's 288 GB; a rank of 8 holds 1/8 of the edges plus its node tables, ghosts counted generously (as many as it
    owns)."""
    hbm = 288e9
    n, k, d, nh, L, world = 4_000_000, 16, 128, 2, 10, 8
    whole = training.edge_training_bytes(n * k, d, d, nh, L)
    assert whole > hbm
    n_owned = n // world
    rank = cdist.shard_edge_training_bytes(n_owned, n_owned, k, d, d, nh, L)
    assert rank < hbm / 3
    assert rank == training.edge_training_bytes(n_owned * k, d, d, nh, L) + 4 * L * 2 * n_owned * d
    assert cdist.shard_edge_training_bytes(n, 0, k, d, d, nh, L) == whole + 4 * L * n * d


def test_edge_row_views_split_on_a_tile():
    t = ops.TiledRows(100, 32, "cpu")
    a = cdist._edge_rows(t, 0, 64)
    b = cdist._edge_rows(t, 64, 100)
    assert (a.n, a.buf.shape[0]) == (64, 64) and (b.n, b.buf.shape[0]) == (36, 64)
    assert a.buf.data_ptr() == t.buf.data_ptr()
    assert b.buf.data_ptr() == t.buf[64].data_ptr()
    whole = cdist._edge_rows(t, 0, 100)
    assert whole.buf.data_ptr() == t.buf.data_ptr() and whole.buf.shape == t.buf.shape
    with pytest.raises(CgnnError):
        cdist._edge_rows(t, 48, 100)          # not on a tile boundary
    with pytest.raises(CgnnError):
        cdist._edge_rows(t, 0, 101)


def _shard(n_owned=40, n_interior=25, k=12):
    z = torch.zeros(n_owned * k, dtype=torch.int32)
    return cdist.Shard(rank=0, world=1, k=k, n_owned=n_owned, n_ghost=0, owned_global=torch.arange(n_owned),
                       ghost_global=torch.zeros(0, dtype=torch.int64), src_local=z, dst_local=z,
                       edge_attr=torch.zeros(n_owned * k, 4), recv_counts=[0], send_idx=torch.zeros(0, dtype=torch.int32),
                       send_counts=[0], n_interior=n_interior)


def test_sharded_training_picks_the_edge_runner():
    model = graph_network.EncodeProcessDecode(32, 32, 2, 2, 3)
    sh = _shard()
    assert type(cdist.ShardedTraining(model, sh)) is cdist.ShardedTraining
    model.message_source = "edge"
    with pytest.raises(NotImplementedError):                   # without the switch, as on one GPU
        cdist.ShardedTraining(model, sh)
    with pytest.raises(NotImplementedError):
        cdist.ShardedEdgeTraining(model, sh)
    model.train_edge_messages = True
    rn = cdist.ShardedTraining(model, sh)
    assert isinstance(rn, cdist.ShardedEdgeTraining)
    assert rn.n_split == 24                                    # 25 interior receivers, k = 12: 24 x 12 = 9 tiles
    model.train_edge_stream = True
    with pytest.raises(NotImplementedError):
        cdist.ShardedTraining(model, sh)
    model.train_edge_stream = False
    sh.batch = torch.zeros(sh.n_owned, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        cdist.ShardedTraining(model, sh)
    model.message_source = "x_j"
    sh.batch = None
    with pytest.raises(NotImplementedError):                   # the edge runner takes edge models only
        cdist.ShardedEdgeTraining(model, sh)
