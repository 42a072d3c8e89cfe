"""GPU: one neighbour search over a batch of independent periodic boxes (``ops.knn_periodic_batched`` /
``cgnn_knn_periodic_batched``) against a loop of the single-graph search (``ops.knn_periodic``) over the graphs: every
row, both edge-feature modes, bit for bit."""
import ctypes as C
import functools

import pytest
import torch

from cosmology_gnn_simulation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = 2.5
GROUP = _lib.KNN_BATCH_GROUP


def _offsets(sizes):
    out = [0]
    for n in sizes:
        out.append(out[-1] + n)
    return out


def _uniform(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand(n, 3, generator=gen) * BOX for n in sizes]


def _cases():
    cases = {"one-graph": _uniform([1000], 1),
             # 5 < k: periodic images of the same particles; 257 and 1000 put graph boundaries inside a workgroup
             "ragged": _uniform([5, 257, 1000], 2)}
    twin = _uniform([300], 3)[0]
    cases["identical-twins"] = [twin, twin.clone()]
    coincident = _uniform([400], 4)[0]
    coincident[100:140] = coincident[7]                       # 41 particles in one place: ties, ordered by local index
    coincident[200:203] = coincident[8]
    cases["coincident"] = [_uniform([50], 5)[0], coincident, _uniform([33], 6)[0]]
    one_cell = 0.31 * BOX + torch.rand(500, 3, generator=torch.Generator().manual_seed(7)) * (BOX / 64)
    cases["one-cell"] = [_uniform([120], 8)[0], one_cell]
    ends = _uniform([600], 9)[0]
    top = float(torch.nextafter(torch.tensor(BOX), torch.tensor(0.0)))
    ends[:200] = torch.where(torch.rand(200, 3, generator=torch.Generator().manual_seed(10)) < 0.5, 0.0, top)
    ends[200:260, 0], ends[260:320, 1], ends[320:380, 2] = 0.0, top, 0.0
    cases["box-ends"] = [ends, _uniform([64], 11)[0]]
    gen = torch.Generator().manual_seed(12)
    sizes = torch.randint(8, 13, (2 * GROUP + 3,), generator=gen).tolist()
    cases["many-graphs"] = _uniform(sizes, 13)
    return cases


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _loop(case, k, min_image):
    """The yardstick, once per case: the single-graph search graph by graph."""
    out = [ops.knn_periodic(p.to(DEV), BOX, k, None, True, True, min_image_edge_attr=min_image) for p in CASES[case]]
    torch.cuda.synchronize()
    return out


# graphs of 8-12 particles are compared at k = 5 and 8 (at k = 16 a miss could only show as a time-out)
PAIRS = [(case, k) for case in CASES for k in (5, 8, 16) if not (case == "many-graphs" and k == 16)]
# the two longer lists of the search kernel (k <= 32, k <= 64): n = 5 among "ragged" gives one sender as several images
PAIRS += [("ragged", 32), ("coincident", 32), ("one-cell", 33), ("ragged", 64)]


@pytest.mark.parametrize("min_image", [False, True], ids=["reference", "image"])
@pytest.mark.parametrize("case,k", PAIRS)
def test_batched_search_gives_the_single_search_bits(case, k, min_image):
    graphs = CASES[case]
    sizes = [p.shape[0] for p in graphs]
    offsets = _offsets(sizes)
    pos = torch.cat(graphs).to(DEV)
    snd, ea, order = ops.knn_periodic_batched(pos, offsets, BOX, k, True, True, min_image_edge_attr=min_image)
    assert snd.dtype == torch.int32 and snd.shape == (offsets[-1] * k,) and ea.shape == (offsets[-1] * k, 4)
    want = _loop(case, k, min_image)
    for g, (a, b) in enumerate(zip(offsets, offsets[1:])):
        mine = snd[a * k:b * k]
        assert int(mine.min()) >= a and int(mine.max()) < b, f"graph {g} reaches outside its rows"
        assert torch.equal(mine - a, want[g][0]), f"senders of graph {g}"
        assert torch.equal(ea[a * k:b * k], want[g][1]), f"edge_attr of graph {g}"
        blk = order[a:b].long()
        assert torch.equal(blk.sort().values, torch.arange(a, b, device=DEV)), f"order of graph {g}"
    # the same senders without edge features or order
    snd2, none_ea, none_order = ops.knn_periodic_batched(pos, offsets, BOX, k, False, False,
                                                         min_image_edge_attr=min_image)
    assert none_ea is None and none_order is None and torch.equal(snd2, snd)


def test_order_follows_each_graphs_own_cells():
    """Block g of ``order`` is cell-sorted: the cell sequence of graph g's single-graph order."""
    graphs = CASES["ragged"]
    offsets = _offsets([p.shape[0] for p in graphs])
    pos = torch.cat(graphs).to(DEV)
    _, _, order = ops.knn_periodic_batched(pos, offsets, BOX, 8, False, True)
    for g, (a, b) in enumerate(zip(offsets, offsets[1:])):
        n = b - a
        _, _, single = ops.knn_periodic(pos[a:b], BOX, 8, None, False, True)
        cells = max(1, min(256, int((n / 2.0) ** (1.0 / 3.0) + 1e-9)))
        inv_h = torch.tensor(float(cells)) / torch.tensor(BOX)      # float32, as the entry computes it

        def cell_ids(idx, a=a, b=b, cells=cells, inv_h=inv_h):
            return (pos[a:b][idx.long()] * inv_h.to(DEV)).floor().clamp(0, cells - 1).long()
        # particles of one cell may come in any order; the cells themselves come in the same sequence
        assert torch.equal(cell_ids(order[a:b] - a), cell_ids(single)), g


@pytest.mark.parametrize("min_image", [False, True], ids=["reference", "image"])
def test_adaptive_grid_gives_the_same_tensors(min_image):
    graphs = CASES["ragged"] + CASES["one-cell"]
    offsets = _offsets([p.shape[0] for p in graphs])
    pos = torch.cat(graphs).to(DEV)
    uni = ops.knn_periodic_batched(pos, offsets, BOX, 8, True, True, min_image_edge_attr=min_image)
    ada = ops.knn_periodic_batched(pos, offsets, BOX, 8, True, True, min_image_edge_attr=min_image, grid="adaptive")
    assert torch.equal(uni[0], ada[0]) and torch.equal(uni[1], ada[1])
    for a, b in zip(offsets, offsets[1:]):
        assert torch.equal(ada[2][a:b].long().sort().values, torch.arange(a, b, device=DEV))


def test_entry_rejects_bad_arguments_and_writes_nothing():
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    n, k = 40, 4
    pos = torch.rand(n, 3, device=DEV)
    sentinel = -7
    snd = torch.full((n * k,), sentinel, dtype=torch.int32, device=DEV)
    ea = torch.full((n * k, 4), float(sentinel), device=DEV)
    perm = torch.full((n,), sentinel, dtype=torch.int32, device=DEV)

    def offs(*values):
        return (C.c_int64 * len(values))(*values)
    good = offs(0, 10, 40)
    ws_bytes = lib.cgnn_knn_batched_workspace_bytes(good, 2, k)
    ws = torch.zeros(ws_bytes + 16, dtype=torch.uint8, device=DEV)

    def run(pos_=pos.data_ptr(), offsets=good, b=2, box=1.0, k_=k, snd_=snd.data_ptr(), ws_=ws.data_ptr(),
            nbytes=ws_bytes, mode=_lib.KNN_EDGE_ATTR_REFERENCE):
        return lib.cgnn_knn_periodic_batched(pos_, offsets, b, box, k_, snd_, ea.data_ptr(), ws_, nbytes, st, mode)
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3      # CGNN_ERR_INVALID_ARG, CGNN_ERR_UNSUPPORTED, CGNN_ERR_WORKSPACE
    assert run(pos_=None) == INVALID and run(offsets=None) == INVALID and run(snd_=None) == INVALID
    assert run(ws_=None) == INVALID and run(k_=0) == INVALID and run(box=0.0) == INVALID
    assert run(ws_=ws.data_ptr() + 4) == INVALID                               # unaligned workspace
    assert run(nbytes=ws_bytes - 256) == WORKSPACE
    assert run(mode=7) == UNSUPPORTED and run(k_=65) == UNSUPPORTED
    many = offs(*range(0, 17 * (2 ** 27 - 1) + 1, 2 ** 27 - 1))                # 17 graphs just under 2^27: 2^31 rows
    assert run(offsets=many, b=16) == WORKSPACE and run(offsets=many, b=17) == UNSUPPORTED
    assert run(offsets=offs(0, 2 ** 27), b=1) == UNSUPPORTED                   # a graph of 2^27 particles
    assert run(b=0) == INVALID and run(b=-1) == INVALID
    assert run(offsets=offs(0, 10, 10), b=2) == INVALID                        # an empty graph
    assert run(offsets=offs(0, 30, 20), b=2) == INVALID                        # offsets that decrease
    assert run(offsets=offs(1, 10, 40), b=2) == INVALID                        # not starting at 0
    assert run(offsets=offs(0, 1, 40), b=2, k_=28) == INVALID                  # k > 27 n_g for the graph of one particle
    assert b"cgnn_knn_periodic_batched" in lib.cgnn_last_error()
    assert lib.cgnn_knn_batched_sorted_order(None, good, 2, perm.data_ptr(), st) == INVALID
    assert lib.cgnn_knn_batched_sorted_order(ws.data_ptr(), good, 2, None, st) == INVALID
    assert lib.cgnn_knn_batched_sorted_order(ws.data_ptr(), offs(0, 10, 10), 2, perm.data_ptr(), st) == INVALID
    assert lib.cgnn_knn_batched_sorted_order(ws.data_ptr(), good, 0, perm.data_ptr(), st) == INVALID
    torch.cuda.synchronize()
    assert bool((snd == sentinel).all()) and bool((ea == sentinel).all()) and bool((perm == sentinel).all())
    assert not bool(ws.any())
    # the valid call of the same arguments runs, and k = 27 n_g is the most a graph of one particle has
    assert run() == 0
    assert run(offsets=offs(0, 1, 40), b=2, k_=4) == 0
    torch.cuda.synchronize()
    assert int(snd.min()) >= 0 and int(snd.max()) < n
