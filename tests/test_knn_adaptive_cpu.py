"""No GPU: the host side of the density-adaptive k-NN grid (``grid="adaptive"`` / ``knn_grid=``): the three C entries
are declared, listed and exported; the workspace figure is O(n) as the header states; unknown grid names are refused
before any device work by every caller; and the argument reaches only build_shard's default search."""
import inspect
import os
import re

import pytest
import torch

from cosmology_gnn_simulation_amd import _lib, data_utils, dist as cdist, ops, rollout, synthetic
from oracle import cpu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cgnn_knn_adaptive_workspace_bytes", "cgnn_knn_periodic_adaptive", "cgnn_knn_adaptive_sorted_order")


def _header():
    return open(os.path.join(ROOT, "include", "cgnn.h")).read()


def test_entries_are_declared_listed_and_exported():
    declared = set(re.findall(r"\b(cgnn_[a-z0-9_]+)\s*\(", _header()))
    lib = _lib.load()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and name in notes
        assert getattr(lib, name).argtypes is not None
    assert lib.cgnn_knn_periodic_adaptive.argtypes == lib.cgnn_knn_periodic.argtypes
    assert lib.cgnn_knn_adaptive_sorted_order.argtypes == lib.cgnn_knn_sorted_order.argtypes
    assert ops.KNN_GRIDS == ("uniform", "adaptive")


def test_workspace_is_linear_in_n_and_covers_the_uniform_one():
    header = _header()
    per = int(re.search(r"#define CGNN_KNN_ADAPTIVE_BYTES_PER_PARTICLE (\d+)", header).group(1))
    fixed = int(re.search(r"#define CGNN_KNN_ADAPTIVE_BYTES_FIXED (\d+)", header).group(1))
    lib = _lib.load()
    ns = sorted(set([1, 2, 3, 5, 15, 16, 17, 53, 54, 127, 128, 129, 1000, 5000, 100_003, 1_000_000, 4_000_000,
                     33_554_431, 33_554_432, 33_554_433, 2 ** 27 - 1] + [2 ** e for e in range(27)] +
                    [2 ** e - 1 for e in range(2, 27)] + [int(1.37 ** e) for e in range(1, 59)]))
    assert ns[0] == 1 and ns[-1] == 2 ** 27 - 1
    last = 0
    for n in ns:
        for k in (1, 16, 64):
            b = lib.cgnn_knn_adaptive_workspace_bytes(n, k)
            assert b == lib.cgnn_knn_adaptive_workspace_bytes(n, 16)          # a function of n alone
            assert b >= lib.cgnn_knn_workspace_bytes(n, k)
            assert b <= per * n + fixed, (n, b)
        assert b >= last, (n, b, last)                                        # monotone in n
        last = b
    assert lib.cgnn_knn_adaptive_workspace_bytes(0, 16) == lib.cgnn_knn_workspace_bytes(0, 16)


def _cpu_window(n=64, w=5):
    snap = synthetic.make_clustered_snapshot(n, w, seed=3)
    return snap["Coordinates"], snap["InternalEnergy"]


class _NoModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, graph):       # pragma: no cover - a refused call never gets here
        raise AssertionError("the model ran")


def test_unknown_grid_names_are_refused_before_any_device_work():
    """CPU tensors, no GPU: anything but the ValueError would be a later failure of the device path."""
    pos = torch.rand(64, 3)
    meta = synthetic.make_metadata()
    c, e = _cpu_window()
    data = {"Coordinates": c, "InternalEnergy": e}
    with pytest.raises(ValueError, match="octree"):
        ops.knn_periodic(pos, 1.0, 8, grid="octree")
    with pytest.raises(ValueError, match="octree"):
        data_utils.knn_graph_periodic(pos, 1.0, 8, grid="octree")
    for noise_rng in ("reference", "device"):
        with pytest.raises(ValueError, match="octree"):
            data_utils.preprocess(c[:5], e[:5], meta, None, None, 0.0, 8, 0.01, 1.0, device="cpu", noise_rng=noise_rng,
                                  knn_grid="octree")
    with pytest.raises(ValueError, match="octree"):
        rollout.rollout(_NoModel(), data, meta, 0.0, 0.01, 1.0, 5, 8, 1, device="cpu", knn_grid="octree")
    with pytest.raises(ValueError, match="octree"):
        cdist.build_shard(pos, 1.0, 8, 2, 0, knn_grid="octree")
    with pytest.raises(ValueError, match="octree"):
        cdist.build_shard(pos, 1.0, 8, 2, 0, knn_fn=_oracle_knn, knn_grid="octree")
    with pytest.raises(ValueError, match="octree"):
        cdist.ShardedRollout(_NoModel(), data, meta, 0.01, 1.0, 5, 8, 1, device="cpu", world=2, rank=0,
                             knn_grid="octree")
    with pytest.raises(ValueError, match="octree"):
        cdist.sharded_rollout(_NoModel(), data, meta, 0.0, 0.01, 1.0, 5, 8, 1, device="cpu", knn_grid="octree")
    with pytest.raises(ValueError, match="octree"):
        cdist.sharded_training_sample(c[:5], e[:5], meta, c[5], e[5], 0.0, 8, 0.01, 1.0, 2, 0, 1, device="cpu",
                                      knn_grid="octree")
    with pytest.raises(ValueError, match="octree"):
        cdist.build_synthetic_shard(64, 2, 0, 8, 1, "cpu", meta, knn_grid="octree")


def test_the_grid_arguments_are_keyword_only_and_default_to_uniform():
    for fn, name in ((ops.knn_periodic, "grid"), (data_utils.knn_graph_periodic, "grid"),
                     (data_utils.preprocess, "knn_grid"), (rollout.rollout, "knn_grid"),
                     (cdist.build_shard, "knn_grid"), (cdist.sharded_training_sample, "knn_grid"),
                     (cdist.ShardedRollout.__init__, "knn_grid"), (cdist.sharded_rollout, "knn_grid"),
                     (cdist.build_synthetic_shard, "knn_grid")):
        params = inspect.signature(fn).parameters
        p = params[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "uniform", fn
        assert list(params)[-1] == name, fn


def _oracle_knn(pos, box, k, query_ids):
    ei, ea = cpu_ref.knn_periodic(pos, box, k)
    q = query_ids.long()
    snd = ei[0].view(pos.shape[0], k)[q].reshape(-1).to(torch.int32)
    attr = ea.view(pos.shape[0], k, 4)[q].reshape(-1, 4)
    return snd, attr, None


@pytest.mark.parametrize("decomposition", ["uniform", "balanced"])
def test_a_callers_own_search_is_left_alone(decomposition):
    pos = synthetic.make_clustered_positions(900, seed=21)
    for rank in range(4):
        a = cdist.build_shard(pos, 1.0, 8, 4, rank, knn_fn=_oracle_knn, decomposition=decomposition)
        b = cdist.build_shard(pos, 1.0, 8, 4, rank, knn_fn=_oracle_knn, decomposition=decomposition,
                              knn_grid="adaptive")
        for name in ("owned_global", "ghost_global", "src_local", "dst_local", "edge_attr"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert a.recv_counts == b.recv_counts and a.n_interior == b.n_interior
