"""CPU: the host logic of sharded training in cosmology_gnn_simulation_amd/dist.py -- the plan of the halo return add and
the reverse all-to-all of ghost-row gradients over gloo (world 2).  The add itself is a HIP kernel in production
(cgnn_halo_return_add); here a torch stand-in follows the plan in the kernel's order."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cosmology_gnn_simulation_amd import dist as cdist
from cosmology_gnn_simulation_amd._lib import CgnnError
from oracle import cpu_ref

N, K, BOX, WORLD = 600, 8, 1.0, 2


def _return_add(table, ret, plan):
    """torch stand-in for ops.halo_return_add: table[rows[j]] += ret[col[p]] for p ascending in row j's segment."""
    rows, seg, col = (t.long() for t in plan)
    for j in range(rows.numel()):
        for p in range(int(seg[j]), int(seg[j + 1])):
            table[rows[j]] += ret[col[p]]
    return table


def test_return_plan_groups_positions_by_row_in_peer_order():
    # peers 0..3; peer 1 sends nothing; rows 5 and 2 are requested by several peers
    send_idx = torch.tensor([5, 2, 9,      # peer 0
                             2, 5, 0,      # peer 2
                             5, 7],        # peer 3
                            dtype=torch.int32)
    rows, seg, col = cdist.halo_return_plan(send_idx, [3, 0, 3, 2], 10)
    assert rows.dtype == seg.dtype == col.dtype == torch.int32
    assert rows.tolist() == [0, 2, 5, 7, 9]
    assert seg.tolist() == [0, 1, 3, 6, 7, 8]
    assert col.tolist() == [5, 1, 3, 0, 4, 6, 7, 2]
    # every position exactly once, each row's positions ascending (= ascending peer rank)
    assert sorted(col.tolist()) == list(range(8))
    for j in range(rows.numel()):
        seg_j = col[seg[j]:seg[j + 1]].tolist()
        assert seg_j == sorted(seg_j) and all(int(send_idx[p]) == int(rows[j]) for p in seg_j)


def test_return_plan_of_a_shard_without_peers_is_empty():
    rows, seg, col = cdist.halo_return_plan(torch.empty(0, dtype=torch.int32), [0, 0, 0], 100)
    assert rows.numel() == 0 and col.numel() == 0 and seg.tolist() == [0]


def test_return_plan_sums_like_the_kernel_order():
    gen = torch.Generator().manual_seed(1)
    send_idx = torch.randint(0, 50, (200,), generator=gen, dtype=torch.int32)
    counts = [40, 0, 60, 100]
    plan = cdist.halo_return_plan(send_idx, counts, 50)
    ret = torch.randn(200, 8, generator=gen, dtype=torch.float64)
    got = _return_add(torch.zeros(50, 8, dtype=torch.float64), ret, plan)
    want = torch.zeros(50, 8, dtype=torch.float64).index_add_(0, send_idx.long(), ret)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("bad,counts", [([0, 3, 10], [3]), ([0, -1, 2], [3]), ([0, 1, 2], [2]), ([0, 1, 2], [4, -1])])
def test_return_plan_rejects_bad_send_lists(bad, counts):
    with pytest.raises(CgnnError):
        cdist.halo_return_plan(torch.tensor(bad, dtype=torch.int32), counts, 10)


def _oracle_knn(pos, box, k, query_ids):
    ei, ea = cpu_ref.knn_periodic(pos, box, k)
    q = query_ids.long()
    snd = ei[0].view(pos.shape[0], k)[q].reshape(-1).to(torch.int32)
    attr = ea.view(pos.shape[0], k, 4)[q].reshape(-1, 4)
    return snd, attr, None


def _positions():
    return torch.rand(N, 3, generator=torch.Generator().manual_seed(78)) * BOX


def _code(rank, gid):
    """The gradient rank ``rank`` sends back for its ghost copy of particle ``gid``: exact in float32, distinct per pair."""
    return 1000.0 * (rank + 1) + gid.to(torch.float32)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pos = _positions()
        sh = cdist.build_shard(pos, BOX, K, world, rank, knn_fn=_oracle_knn)
        sh = cdist.exchange_requests(sh)
        halo = cdist.HaloExchange(sh, pack_fn=lambda t, idx, out: out.copy_(t[idx.long()]))
        width = 4
        cols = torch.tensor([0.0, 0.25, 0.5, 0.75])
        # the gradient of every ghost row of [n_owned, n_local): a value that encodes (this rank, global id)
        grad_ghost = (_code(rank, sh.ghost_global).view(-1, 1) + cols).contiguous()
        handle = halo.start_return(grad_ghost)
        busy = torch.randn(64, 64) @ torch.randn(64, 64)          # work under the exchange
        ret = halo.finish_return(handle)
        ok_shape = tuple(ret.shape) == (sum(sh.send_counts), width)
        # position p of the return carries the gradient of owned row send_idx[p], from the peer it was sent to
        peer_of = torch.repeat_interleave(torch.arange(world), torch.tensor(sh.send_counts))
        gid_of = sh.owned_global[sh.send_idx.long()]
        ok_rows = torch.equal(ret, _code(peer_of, gid_of).view(-1, 1) + cols)
        base = sh.owned_global.to(torch.float32).view(-1, 1) * 0.5 + cols
        dx = _return_add(base.clone(), ret, cdist.halo_return_plan(sh.send_idx, sh.send_counts, sh.n_owned))
        # independent oracle: every other rank's shard, rebuilt here; the owner receives the code of each rank
        # that holds the particle as a ghost
        want = base.clone()
        for p in range(world):
            if p == rank:
                continue
            other = cdist.build_shard(pos, BOX, K, world, p, knn_fn=_oracle_knn)
            g2l = torch.full((N,), -1, dtype=torch.long)
            g2l[sh.owned_global] = torch.arange(sh.n_owned)
            mine = other.ghost_global[g2l[other.ghost_global] >= 0]
            want[g2l[mine]] += _code(p, mine).view(-1, 1) + cols
        touched = int((dx != base).any(dim=1).sum())
        q.put((rank, ok_shape, ok_rows, bool(torch.equal(dx, want)), touched, sh.n_ghost, sum(sh.send_counts),
               bool(torch.isfinite(busy).all())))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(120)
def test_reverse_exchange_returns_ghost_gradients_to_their_owners_over_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=100) for _ in procs)
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    for rank, ok_shape, ok_rows, ok_sum, touched, n_ghost, n_sent, ok_busy in res:
        assert ok_shape and ok_rows and ok_sum and ok_busy, rank
        assert n_ghost > 0 and 0 < touched <= n_sent
    assert res[0][6] == res[1][5] and res[1][6] == res[0][5]      # rows returned == ghost rows the peer sent back
