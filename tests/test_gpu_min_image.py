"""GPU: minimum-image edge features (``min_image_edge_attr=True``; cgnn_knn_periodic_mode and
cgnn_knn_periodic_adaptive_mode with CGNN_KNN_EDGE_ATTR_IMAGE) through every caller that takes the keyword.

The oracle is tests/min_image_checks.py: the reference's ``extended_positions[ext_idx] - recent_position[receiver]``.
Gates (those of tests/test_gpu_knn_adaptive.py::_against_oracle): ``torch.equal`` on senders and on the three
displacement columns, the norm within 1e-6 box; bit for bit between the two grids and between two runs.  Model outputs:
``TOL`` of tests/test_gpu_parity.py; gradients: ``GTOL`` of tests/test_gpu_training_edge.py."""
import numpy as np
import pytest
import torch

import min_image_checks as mic
from conftest import rel_err
from cosmology_gnn_simulation_amd import data_utils, dist as cdist, graph_network, ops, rollout, synthetic
from cosmology_gnn_simulation_amd.graph import Data
from cosmology_gnn_simulation_amd.one_step import integrate_one_step, integration_constants
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5      # tests/test_gpu_parity.py


# ---- the k-NN itself ------------------------------------------------------------------------------------------------------

def _both_grids(pos, box, k, query_ids=None):
    """Image mode on both grids, twice each: identical bits; senders those of the default mode.  -> (senders, attr)."""
    p = pos.to(DEV)
    q = None if query_ids is None else query_ids.to(DEV)
    out = None
    for grid in ops.KNN_GRIDS:
        s0, a0, _ = ops.knn_periodic(p, box, k, query_ids=q, grid=grid)
        s1, a1, _ = ops.knn_periodic(p, box, k, query_ids=q, grid=grid, min_image_edge_attr=True)
        s2, a2, _ = ops.knn_periodic(p, box, k, query_ids=q, grid=grid, min_image_edge_attr=True)
        assert torch.equal(s1, s0), grid                                   # the default mode's senders
        assert torch.equal(s2, s1) and torch.equal(a2, a1), grid           # two runs
        assert a1.shape == a0.shape
        if out is not None:
            assert torch.equal(s1, out[0]) and torch.equal(a1, out[1])     # the two grids
        out = (s1, a1)
    return out[0], out[1], a0


def _against_oracle(pos, box, k, query_ids=None):
    n = pos.shape[0]
    ei, ea, image = mic.min_image_graph(pos, box, k)
    want_s, want_a, image = ei[0].view(n, k), ea.view(n, k, 4), image.view(n, k)
    if query_ids is not None:
        want_s, want_a, image = want_s[query_ids.long()], want_a[query_ids.long()], image[query_ids.long()]
    snd, attr, attr_ref = _both_grids(pos, box, k, query_ids)
    want_a = want_a.reshape(-1, 4)
    assert torch.equal(snd.cpu().long(), want_s.reshape(-1))
    assert torch.equal(attr.cpu()[:, :3], want_a[:, :3])
    assert torch.allclose(attr.cpu(), want_a, rtol=0, atol=1e-6 * box)
    centre = (image == mic.CENTRE).reshape(-1)
    assert torch.equal(attr.cpu()[centre], attr_ref.cpu()[centre])          # centre rows: the default mode's bits
    return attr.cpu(), centre


@pytest.mark.parametrize("n,k,box,seed", mic.SHAPES)
def test_min_image_uniform_boxes_bit_exact(n, k, box, seed):
    attr, centre = _against_oracle(mic.uniform_positions(n, box, seed), box, k)
    assert bool((~centre).any())
    if n >= 256:
        assert float(attr[:, :3].abs().max()) < box / 2


def _clumps():
    """The input of tests/test_gpu_parity.py::test_knn_clustered_positions_bit_exact."""
    gen = torch.Generator().manual_seed(17)
    centers = torch.rand(12, 3, generator=gen)
    centers[0] = torch.tensor([0.999, 0.001, 0.5])                  # a clump on the box corner/edge
    clumps = (centers.repeat_interleave(250, 0) + 0.004 * torch.randn(3000, 3, generator=gen)) % 1.0
    return torch.cat([clumps, torch.rand(500, 3, generator=gen)]).float()


@pytest.mark.parametrize("k", [8, 16])
def test_min_image_clumps_bit_exact(k):
    attr, centre = _against_oracle(_clumps(), 1.0, k)
    assert bool((~centre).any()) and float(attr[:, :3].abs().max()) < 0.5


def test_min_image_coordinates_on_the_box_faces():
    """The input of tests/test_gpu_knn_adaptive.py::test_adaptive_coordinates_on_the_box_faces."""
    gen = torch.Generator().manual_seed(21)
    box = 1.0
    top = float(np.nextafter(np.float32(box), np.float32(0)))
    pos = torch.rand(4000, 3, generator=gen)
    pos[:300] = torch.clamp((0.002 * torch.randn(300, 3, generator=gen)) % 1.0, max=top)
    pos[300:600] = torch.clamp(pos[300:600] * 0.004 + 0.996, max=top)
    pos[0] = torch.tensor([0.0, 0.0, 0.0])
    pos[1] = torch.tensor([top, top, top])
    pos[2] = torch.tensor([0.0, top, 0.5])
    pos[3] = torch.tensor([top, 0.0, 0.0])
    for k in (8, 16):
        _against_oracle(pos, box, k)


def test_min_image_query_subset_and_coincident_pair():
    gen = torch.Generator().manual_seed(9)
    pos = torch.rand(500, 3, generator=gen)
    pos[10] = pos[3]                                               # coincident particles: tie broken by index
    _against_oracle(pos, 1.0, 8)
    _against_oracle(pos, 1.0, 8, torch.tensor([3, 10, 499, 0], dtype=torch.int32))
    # queries next to the faces, inside refined cells: a halo moved onto the box corner, one coincident pair in its core
    pos = torch.remainder(synthetic.make_clustered_positions(20_000, seed=6) - 0.25, 1.0)
    core = torch.argsort(torch.minimum(pos, 1.0 - pos).norm(dim=1))[:2]
    pos[core[1]] = pos[core[0]]
    q = torch.cat([core, torch.arange(0, 20_000, 37)]).to(torch.int32)
    _, centre = _against_oracle(pos, 1.0, 8, q)
    assert bool((~centre).any())


def test_min_image_fewer_particles_than_neighbours():
    """Several images of one particle among a receiver's neighbours: only the ranked image tells them apart."""
    pos = mic.uniform_positions(5, 1.0, 5)
    attr, _ = _against_oracle(pos, 1.0, 8)
    snd = ops.knn_periodic(pos.to(DEV), 1.0, 8, want_edge_attr=False)[0].view(5, 8).cpu()
    rows = attr.view(5, 8, 4)
    twice = 0
    for i in range(5):
        for a in range(8):
            for b in range(a + 1, 8):
                if snd[i, a] == snd[i, b]:
                    twice += 1
                    assert not torch.equal(rows[i, a], rows[i, b])
    assert twice > 0
    _against_oracle(mic.uniform_positions(40, 1.0, 4), 1.0, 32)


def test_min_image_clustered_100k_grids_agree():
    pos = synthetic.make_clustered_positions(100_003, seed=2)
    snd, attr, attr_ref = _both_grids(pos, 1.0, 16)
    assert float(attr[:, :3].abs().max()) < 0.5 < float(attr_ref[:, :3].abs().max())
    same = (attr == attr_ref).all(dim=1)
    assert 0.0 < float((~same).float().mean()) < 0.2
    # a row either is the default mode's or differs from it by whole boxes
    moved = ((attr[:, :3] - attr_ref[:, :3]).abs() > 0.5).any(dim=1)
    assert torch.equal(moved, ~same)


def test_an_unknown_mode_is_unsupported():
    from cosmology_gnn_simulation_amd import _lib
    lib = _lib.load()
    n, k = 1000, 8
    pos = torch.rand(n, 3, device=DEV)
    snd = torch.empty(n * k, dtype=torch.int32, device=DEV)
    for entry, ws_fn in ((lib.cgnn_knn_periodic_mode, lib.cgnn_knn_workspace_bytes),
                         (lib.cgnn_knn_periodic_adaptive_mode, lib.cgnn_knn_adaptive_workspace_bytes)):
        nbytes = ws_fn(n, k)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        args = (pos.data_ptr(), n, 1.0, k, None, n, snd.data_ptr(), None, ws.data_ptr(), nbytes, None)
        assert entry(*args, 2) == -2 and entry(*args, -1) == -2        # CGNN_ERR_UNSUPPORTED
        assert entry(*args[:9], nbytes - 1, None, 1) == -3             # CGNN_ERR_WORKSPACE, as the old entries
        assert entry(*args, 0) == 0 and entry(*args, 1) == 0
    torch.cuda.synchronize()


# ---- preprocess -------------------------------------------------------------------------------------------------------------

W = 5


@pytest.mark.parametrize("noise_rng", ["reference", "device"])
@pytest.mark.parametrize("knn_grid", ops.KNN_GRIDS)
def test_preprocess_changes_the_edge_features_only(noise_rng, knn_grid):
    n, k = 6000, 16
    snap = synthetic.make_clustered_snapshot(n, W, seed=51)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    graphs = []
    for flag in (False, True):
        torch.manual_seed(5)
        graphs.append(data_utils.preprocess(c[:W].clone(), e[:W].clone(), meta, c[W].clone(), e[W].clone(), 3e-4, k,
                                            0.01, 1.0, device=DEV, noise_rng=noise_rng, noise_seed=77, noise_draw=3,
                                            knn_grid=knn_grid, min_image_edge_attr=flag))
    off, on = graphs
    for name in ("x", "edge_index", "pos", "y_acc", "y_temp_rate"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    ei, ea, image = mic.min_image_graph(on.pos.cpu(), 1.0, k)
    assert torch.equal(on.edge_index.cpu(), ei)
    assert torch.equal(on.edge_attr.cpu()[:, :3], ea[:, :3])
    assert torch.allclose(on.edge_attr.cpu(), ea, rtol=0, atol=1e-6)
    assert not torch.equal(on.edge_attr, off.edge_attr)


# ---- models -----------------------------------------------------------------------------------------------------------------

def _translation_model(msg):
    m = graph_network.EncodeProcessDecode(*mic.T_MODEL)
    m.load_state_dict(synthetic.make_state_dict(*mic.T_MODEL))
    m = m.to(DEV).eval()
    m.message_source = msg
    return m


def _device_graph(x, pos, flag):
    ei, ea, _, _ = data_utils.knn_graph_periodic(pos.to(DEV), mic.T_BOX, mic.T_K, min_image_edge_attr=flag)
    return Data(x=x.to(DEV), edge_index=ei, edge_attr=ea)


def test_a_translation_leaves_an_edge_model_alone():
    """Default precisions, message_source="edge", N = 2000, k = 16: the box translated by (0.37, 0.81, 0.55) mod 1."""
    sd, x, pos, moved = mic.translation_problem()
    model = _translation_model("edge")
    got, want = [], []
    with torch.no_grad():
        for p in (pos, moved):
            g = _device_graph(x, p, True)
            got.append({key: v.cpu() for key, v in model(g).items()})
            want.append(mic.oracle_outputs(sd, x, g.edge_index.cpu(), g.edge_attr.cpu(), "edge"))
        off = [{key: v.cpu() for key, v in model(_device_graph(x, p, False)).items()} for p in (pos, moved)]
    for key in ("acceleration", "temp_rate"):
        for g_, w_ in zip(got, want):
            err = rel_err(g_[key], w_[key])
            print(f"{key}: device against the oracle on the same graph {err:.3e}")
            assert err <= TOL, key
        # |d_a - d_b| <= |d_a - o_a| + |o_a - o_b| + |o_b - d_b|, the outer two bounded by the assertion above
        oracle_change = float((want[0][key] - want[1][key]).abs().max())
        bound = TOL * (float(want[0][key].abs().max()) + float(want[1][key].abs().max())) + oracle_change
        change = float((got[0][key] - got[1][key]).abs().max())
        print(f"{key}: device change {change:.3e}, oracle change {oracle_change:.3e}, bound {bound:.3e}; relative "
              f"{mic.rel_max_change(got[0][key], got[1][key]):.3e}; flag off {mic.rel_max_change(off[0][key], off[1][key]):.3e}")
        assert change <= bound, key
        assert mic.rel_max_change(off[0][key], off[1][key]) > 1e-2, key


def test_an_x_j_model_does_not_read_the_edge_features():
    n, k = 3000, 16
    snap = synthetic.make_snapshot(n, W, seed=8)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    model = graph_network.EncodeProcessDecode(64, 64, 2, 3, 3)
    model.load_state_dict(synthetic.make_state_dict(64, 64, 2, 3, 3))
    model = model.to(DEV).eval()
    assert model.message_source == "x_j"
    outs = []
    with torch.no_grad():
        for flag in (False, True):
            g = data_utils.preprocess(c[:W], e[:W], meta, None, None, 0.0, k, 0.01, 1.0, device=DEV,
                                      min_image_edge_attr=flag)
            outs.append(model(g))
    for key in ("acceleration", "temp_rate"):
        assert torch.equal(outs[0][key], outs[1][key]), key


# ---- rollouts ---------------------------------------------------------------------------------------------------------------

def _rollout_problem(n, seed, clustered=False):
    import test_gpu_balanced_decomposition as tbd
    import test_gpu_sharded_rollout as tsr
    data = tbd._clustered_window(n, seed=seed) if clustered else tsr._window(n, seed=seed)
    return tsr, data, tsr._model(64, 3, "edge", "fp32", seed=9), synthetic.make_metadata(tsr.BOX, tsr.DT)


def test_rollout_is_the_loop_of_preprocess_model_and_integration():
    n, k, steps = 6000, 16, 4
    tsr, data, model, meta = _rollout_problem(n, 71)
    w, dt, box = tsr.W, tsr.DT, tsr.BOX
    with torch.no_grad():
        got = rollout.rollout(model, data, meta, 0.0, dt, box, w, k, steps, min_image_edge_attr=True)
        off = rollout.rollout(model, data, meta, 0.0, dt, box, w, k, steps)
        pos = torch.empty((w + steps, n, 3), device=DEV)
        tmp = torch.empty((w + steps, n, 1), device=DEV)
        pos[:w], tmp[:w] = data["Coordinates"][:w].to(DEV).float(), data["InternalEnergy"][:w].to(DEV).float()
        m = dict(meta)
        m["dt"], m["box_size"] = dt, box
        consts = integration_constants(m, torch.device(DEV))
        for t in range(w, w + steps):
            g = data_utils.preprocess(pos[t - w:t], tmp[t - w:t], m, None, None, 0.0, k, dt, box, device=DEV,
                                      reference_rng=False, check_bounds=False, min_image_edge_attr=True)
            pred = model(g)
            pos[t], tmp[t] = integrate_one_step(pred["acceleration"], pred["temp_rate"], pos[t - w:t], tmp[t - w:t], m,
                                                consts)
    assert torch.equal(got["Coordinates"], pos) and torch.equal(got["InternalEnergy"], tmp)
    assert bool(torch.isfinite(pos).all())
    assert torch.equal(got["Coordinates"][:w], off["Coordinates"][:w])
    assert not torch.equal(got["Coordinates"][w], off["Coordinates"][w])
    assert not torch.equal(got["InternalEnergy"][-1], off["InternalEnergy"][-1])


def test_validate_one_step_passes_the_flag_on():
    from cosmology_gnn_simulation_amd import one_step
    n, k = 3000, 16
    tsr, data, model, meta = _rollout_problem(n, 73)
    w = tsr.W
    m = dict(meta)
    m["dt"], m["box_size"] = tsr.DT, tsr.BOX
    snap = {"Coordinates": torch.remainder(data["Coordinates"], tsr.BOX),
            "InternalEnergy": data["InternalEnergy"]}
    snap = {key: torch.cat([v, v[-1:]]) for key, v in snap.items()}         # W + 1 frames: one window and its target
    on = one_step.validate_one_step(model, snap, m, w, DEV, k, start_indices=[0], min_image_edge_attr=True)
    off = one_step.validate_one_step(model, snap, m, w, DEV, k, start_indices=[0])
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    with torch.no_grad():
        g = data_utils.preprocess(c[:w].float(), e[:w].float(), m, noise_std=0.0, num_neighbors=k, box_size=tsr.BOX,
                                  dt=tsr.DT, device=DEV, min_image_edge_attr=True)
        pred = model(g)
    new_p, _ = integrate_one_step(pred["acceleration"], pred["temp_rate"], c[:w].float(), e[:w].float(), m)
    assert on["position_error"] == torch.mean((new_p - c[w].to(DEV)) ** 2).item()
    assert on["position_error"] != off["position_error"]


# ---- sharded paths ----------------------------------------------------------------------------------------------------------

WORLDS = (2, 8)
DECOMPOSITIONS = ("uniform", "balanced")


@pytest.mark.parametrize("decomposition", DECOMPOSITIONS)
@pytest.mark.parametrize("world", WORLDS)
def test_shards_carry_the_one_gpu_rows(world, decomposition):
    n, k = 20_000, 16
    pos = synthetic.make_clustered_positions(n, seed=5).to(DEV)
    snd, want, _ = ops.knn_periodic(pos, 1.0, k, min_image_edge_attr=True)
    want, snd = want.view(n, k, 4), snd.view(n, k).long()
    seen = torch.zeros(n, dtype=torch.int32, device=DEV)
    differ = 0
    for r in range(world):
        for grid in ops.KNN_GRIDS:
            sh = cdist.build_shard(pos, 1.0, k, world, r, decomposition=decomposition, knn_grid=grid,
                                   min_image_edge_attr=True)
            assert torch.equal(sh.edge_attr.view(sh.n_owned, k, 4), want[sh.owned_global])
            table = torch.cat([sh.owned_global, sh.ghost_global])
            assert torch.equal(table[sh.src_local.long()].view(sh.n_owned, k), snd[sh.owned_global])
        # the default mode's shard: the same rows (the local order inside a cell of the search grid is not fixed from
        # one search to the next, so rows are compared in ascending id), other features on the crossing edges
        ref = cdist.build_shard(pos, 1.0, k, world, r, decomposition=decomposition)
        a, b = torch.argsort(sh.owned_global), torch.argsort(ref.owned_global)
        assert torch.equal(ref.owned_global[b], sh.owned_global[a])
        assert torch.equal(ref.ghost_global, sh.ghost_global) and ref.recv_counts == sh.recv_counts
        differ += int((ref.edge_attr.view(-1, k, 4)[b] != sh.edge_attr.view(-1, k, 4)[a]).any(dim=2).sum())
        seen[sh.owned_global] += 1
    assert bool((seen == 1).all()) and differ > 0


@pytest.mark.parametrize("decomposition", DECOMPOSITIONS)
@pytest.mark.parametrize("world", WORLDS)
def test_sharded_training_sample_carries_the_one_gpu_rows(world, decomposition):
    import noise_checks as nc
    n, k, w = 20_011, 16, 5
    meta = nc.rich_metadata()
    dt, box = meta["dt"], meta["box_size"]
    snap = synthetic.make_clustered_snapshot(n, w, box_size=box, dt=dt, seed=31)
    pos, tmp = snap["Coordinates"][:w].to(DEV), snap["InternalEnergy"][:w].to(DEV)
    tp, tt = snap["Coordinates"][w].to(DEV), snap["InternalEnergy"][w].to(DEV)
    noise_std, seed, draw = 3e-4, 2 ** 32 + 977, 2 ** 32 + 9
    g = data_utils.preprocess(pos, tmp, meta, tp, tt, noise_std, k, dt, box, device=DEV, noise_rng="device",
                              noise_seed=seed, noise_draw=draw, min_image_edge_attr=True)
    want = g.edge_attr.view(n, k, 4)
    ei, ea, _ = mic.min_image_graph(g.pos.cpu(), box, k)
    assert torch.equal(g.edge_index.cpu(), ei) and torch.equal(g.edge_attr.cpu()[:, :3], ea[:, :3])
    for rank in range(world):
        sh = cdist.sharded_training_sample(pos, tmp, meta, tp, tt, noise_std, k, dt, box, world, rank, seed, draw,
                                           decomposition=decomposition, min_image_edge_attr=True)
        assert torch.equal(sh.edge_attr.view(sh.n_owned, k, 4), want[sh.owned_global])
        assert torch.equal(sh.x_feat, g.x[sh.owned_global]) and torch.equal(sh.y_acc, g.y_acc[sh.owned_global])


def _loopback_replicated(tsr, model, data, meta, world, k, steps, decomposition):
    """tests/test_gpu_knn_adaptive.py's loopback rollout with the flag on."""
    runners = [cdist.ShardedRollout(model, data, meta, tsr.DT, tsr.BOX, tsr.W, k, steps, world=world, rank=r,
                                    decomposition=decomposition, min_image_edge_attr=True) for r in range(world)]
    with torch.no_grad():
        for t in range(tsr.W, tsr.W + steps):
            shards = [rn.plan(t) for rn in runners]
            for r, sh in enumerate(shards):
                cdist.finish_shard(sh, [shards[p].want_global[r] for p in range(world)])
                runners[r].features(sh, t)
            preds = tsr._loopback_forward([rn.forward(sh, halo=lambda table: None) for rn, sh in zip(runners, shards)],
                                          shards)
            gathered = torch.cat([rn.integrate(sh, p, t) for rn, sh, p in zip(runners, shards, preds)])
            for rn in runners:
                rn.publish(gathered, t)
    return [rn.result() for rn in runners]


def _loopback_owned(tsr, model, data, meta, world, k, steps, decomposition):
    """tests/test_gpu_migrating_rollout.py's loopback (every rank's MigratingRollout in one process, the exchanges as
    slices and concatenations) with the flag on."""
    w, dt, box = tsr.W, tsr.DT, tsr.BOX
    n = data["Coordinates"].shape[1]
    coords, energy = data["Coordinates"][:w], data["InternalEnergy"][:w]
    _, recent = ops.window_features(coords[w - 2:].to(DEV), energy[w - 2:].to(DEV), meta, dt, box)
    planes = cdist.balanced_planes(recent, box, world) if decomposition == "balanced" else None
    owner0 = cdist.owner_of(recent, box, world, planes).cpu()
    runners = []
    for r in range(world):
        ids = torch.nonzero(owner0 == r).squeeze(1)
        runners.append(cdist.MigratingRollout(model, ids, coords[:, ids], energy[:, ids], n_total=n, metadata=meta, dt=dt,
                                              box_size=box, window_size=w, num_neighbors=k, num_steps=steps, device=DEV,
                                              world=world, rank=r, planes=planes, min_image_edge_attr=True))
    with torch.no_grad():
        for _ in range(steps):
            for rn in runners:
                rn.begin()
            while True:
                outs = [rn.halo_out() for rn in runners]
                failed = []
                for r, rn in enumerate(runners):
                    blocks, counts = [], []
                    for p in range(world):
                        rows_p, sc = outs[p]
                        start = sum(sc[:r])
                        blocks.append(rows_p[start:start + sc[r]])
                        counts.append(sc[r])
                    failed.append(rn.search(torch.cat(blocks), counts))
                if not any(failed):
                    break
                for rn in runners:
                    rn.widen()
            shards = [rn.number() for rn in runners]
            for r, sh in enumerate(shards):
                cdist.finish_shard_by_search(sh, [shards[p].want_global[r] for p in range(world)])
                runners[r].features(sh)
            preds = tsr._loopback_forward([rn.forward(sh, halo=lambda table: None) for rn, sh in zip(runners, shards)],
                                          shards)
            sends = [rn.advance(p) for rn, p in zip(runners, preds)]
            leavers = [rn.migrate_out(sum(sends[p][r] for p in range(world))) for r, rn in enumerate(runners)]
            for r, rn in enumerate(runners):
                blocks = []
                for p in range(world):
                    start = sum(sends[p][:r])
                    blocks.append(leavers[p][start:start + sends[p][r]])
                rn.receive(torch.cat(blocks))
            held = sum(rn.n_held for rn in runners)
            for rn in runners:
                rn.check_total(held)
    return cdist.assemble_frames([rn.result() for rn in runners], n)


@pytest.mark.parametrize("decomposition", DECOMPOSITIONS)
@pytest.mark.parametrize("world", WORLDS)
def test_loopback_sharded_rollouts_give_the_one_gpu_frames(world, decomposition):
    n, k, steps = 6000, 16, 3
    tsr, data, model, meta = _rollout_problem(n, 80 + world, clustered=decomposition == "balanced")
    with torch.no_grad():
        want = rollout.rollout(model, data, meta, 0.0, tsr.DT, tsr.BOX, tsr.W, k, steps, min_image_edge_attr=True)
        off = rollout.rollout(model, data, meta, 0.0, tsr.DT, tsr.BOX, tsr.W, k, steps)
    assert bool(torch.isfinite(want["Coordinates"]).all())
    assert not torch.equal(want["Coordinates"][tsr.W], off["Coordinates"][tsr.W])
    for got in _loopback_replicated(tsr, model, data, meta, world, k, steps, decomposition):
        assert torch.equal(got["Coordinates"], want["Coordinates"])
        assert torch.equal(got["InternalEnergy"], want["InternalEnergy"])
    got = _loopback_owned(tsr, model, data, meta, world, k, steps, decomposition)
    assert torch.equal(got["Coordinates"], want["Coordinates"])
    assert torch.equal(got["InternalEnergy"], want["InternalEnergy"])


@pytest.mark.parametrize("decomposition", DECOMPOSITIONS)
@pytest.mark.parametrize("storage", ["replicated", "owned"])
def test_the_sharded_rollout_driver_passes_the_flag_on(storage, decomposition):
    """A world of one (no process group) through ``sharded_rollout`` itself, both storages."""
    n, k, steps = 3000, 16, 3
    tsr, data, model, meta = _rollout_problem(n, 77)
    with torch.no_grad():
        want = rollout.rollout(model, data, meta, 0.0, tsr.DT, tsr.BOX, tsr.W, k, steps, min_image_edge_attr=True)
        off = rollout.rollout(model, data, meta, 0.0, tsr.DT, tsr.BOX, tsr.W, k, steps)
    got = cdist.sharded_rollout(model, data, meta, 0.0, tsr.DT, tsr.BOX, tsr.W, k, steps, decomposition=decomposition,
                                storage=storage, min_image_edge_attr=True)
    if storage == "owned":
        got = cdist.assemble_frames([got], n)
    assert torch.equal(got["Coordinates"], want["Coordinates"])
    assert torch.equal(got["InternalEnergy"], want["InternalEnergy"])
    assert not torch.equal(got["Coordinates"], off["Coordinates"])


# ---- training ---------------------------------------------------------------------------------------------------------------

def test_an_edge_mode_training_step_on_a_minimum_image_graph():
    """tests/test_gpu_training_edge.py's well-conditioned shape (600, 8, 32, 2, 2) and its gates, on a graph built with
    the flag on: nothing downstream of the graph build assumes the reference's features."""
    import test_gpu_training_edge as tte
    n, k, latent, nh, steps, window, dt = 600, 8, 32, 2, 2, 5, 0.01
    snap = synthetic.make_snapshot(n, window, seed=n)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    g = data_utils.preprocess(c[:window].clone(), e[:window].clone(), meta, c[window].clone(), e[window].clone(), 0.0, k,
                              dt, 1.0, min_image_edge_attr=True)
    _, ea, image = mic.min_image_graph(g.pos.cpu(), 1.0, k)
    assert torch.equal(g.edge_attr.cpu()[:, :3], ea[:, :3]) and bool((image != mic.CENTRE).any())
    sd = synthetic.make_state_dict(latent, latent, nh, steps, 3, node_in=g.x.shape[1], edge_in=4, seed=n + 1)
    want_loss, sdr, want_dx, want_dea, want_out = tte._reference(sd, g, nh, steps, dt)
    model = tte._edge_model(latent, nh, steps, sd)
    g.x.requires_grad_(True)
    g.edge_attr.requires_grad_(True)
    pred = model(g)
    loss = tte._loss(pred, g, dt)
    loss.backward()
    assert tte._close(pred["acceleration"], want_out["acceleration"], 1e-5)
    assert tte._close(pred["temp_rate"], want_out["temp_rate"], 1e-5)
    assert abs(float(loss.detach()) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    assert tte._close(g.x.grad, want_dx, tte.GTOL)
    assert g.edge_attr.grad is not None and tte._close(g.edge_attr.grad, want_dea, tte.GTOL)
    got = dict(model.named_parameters())
    for name, ref in sdr.items():
        assert ref.grad is not None and got[name].grad is not None, name
        # one-element gradients (the temperature decoder's output bias): as in tests/test_gpu_training_edge.py
        assert tte._close(got[name].grad, ref.grad, tte.GTOL if ref.grad.numel() > 1 else 5 * tte.GTOL), name
