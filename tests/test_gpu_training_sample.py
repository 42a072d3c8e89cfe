"""GPU: cgnn_training_sample -- a training sample with noise made on the device -- and its callers
``data_utils.preprocess(noise_rng="device")`` and ``dist.sharded_training_sample``.

The normals are checked against the float64 restatement of tests/noise_checks.py in units of one normal; everything
downstream of the noise is checked bit for bit against the CPU oracle fed with the kernel's own noise."""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_checks as nc
from conftest import load_golden
from cosmology_gnn_simulation_amd import _lib, data_utils, dist as cdist, ops, synthetic
from cosmology_gnn_simulation_amd._lib import CgnnError
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOISE_STD = 3e-4
SEEDS = (20240229, 2 ** 32 + 977)
DRAWS = (0, 2 ** 32 + 1)

# Largest deviation of the kernel's walk from the float64 restatement, in units of one normal (test_noise_...):
# measured on an MI355X over W in {2, 5, 6, 16}, both seeds, both draws, 100 003 particles: NOISE_MEASURED.  The gate is
# 4 x that: the error of logf / sincospif / sqrtf grows with |z| and other seeds reach further into the tail.  It must
# stay below 1e-5: one grid step of a uniform moves a normal by up to 2 pi 2^-23 5.77 = 4.3e-6, so 1e-5 would no longer
# be function rounding but another uniform or an approximate function.
NOISE_MEASURED = 8.0e-7
NOISE_GATE = 4 * NOISE_MEASURED          # 3.2e-6


def _window(n, w, seed, box=1.0):
    snap = synthetic.make_snapshot(n, w, seed=seed)
    c, e = snap["Coordinates"].float() * box, snap["InternalEnergy"].float()
    return c[:w].contiguous(), e[:w].contiguous(), c[w].contiguous(), e[w].contiguous()


def _noise(pos, tmp, meta, seed, draw, rows=None, noise_std=NOISE_STD):
    out = ops.training_sample(pos, tmp, meta, meta["dt"], meta["box_size"], noise_std, seed, draw, rows=rows,
                              want=("pos_noise", "temp_noise"))
    return out["pos_noise"], out["temp_noise"]


# ---- 5: the noise against the restatement ------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [2, 5, 6, 16])
def test_noise_is_the_restated_walk(w):
    """Kernel noise against Philox + float64 Box-Muller + float64 walk of tests/noise_checks.py, in units of one normal
    (difference / (step scale x dt) / (S (S + 1) / 2)).  Measured on an MI355X: 8.0e-7 (W = 2), 5.0e-7 (W = 5), 3.7e-7
    (W = 6), 1.6e-7 (W = 16); the gate is 4 x the largest, 3.2e-6 (NOISE_MEASURED / NOISE_GATE above)."""
    n = 100_003                                     # not a multiple of the block
    meta = nc.rich_metadata()
    dt, trs = meta["dt"], meta["temp_rate_std"]
    pos, tmp, _, _ = _window(n, w, seed=7)
    pos, tmp = pos.to(DEV), tmp.to(DEV)
    ids = np.arange(n)
    rows = torch.from_numpy(np.random.default_rng(w).permutation(n)[:4097].copy()).to(DEV)
    worst = 0.0
    for seed in SEEDS:
        for draw in DRAWS:
            pn, tn = _noise(pos, tmp, meta, seed, draw)
            assert pn.shape == (n, w, 3) and tn.shape == (n, w)
            assert not pn[:, 0].any() and not tn[:, 0].any()                  # frame 0 carries no noise
            want_p, want_t = nc.walk_f64(nc.normals_window(ids, w, seed, draw), NOISE_STD, trs, dt)
            dev = nc.normal_units(pn.cpu().double().numpy() - want_p, tn.cpu().double().numpy() - want_t, w,
                                  NOISE_STD, trs, dt)
            print(f"W={w} seed={seed} draw={draw}: largest deviation {dev:.3e} normals")
            worst = max(worst, dev)
            pn_r, tn_r = _noise(pos, tmp, meta, seed, draw, rows=rows)
            assert torch.equal(pn_r, pn[rows]) and torch.equal(tn_r, tn[rows])   # a subset: the same bits
        # another seed or draw is another sample
        other = _noise(pos, tmp, meta, seed, DRAWS[0])[0]
        assert not torch.equal(other, pn)
    print(f"W={w}: largest deviation over seeds and draws {worst:.3e} normals (gate {NOISE_GATE})")
    assert worst < 2.5e-6, "above 2.5e-6 the 4 x gate would pass 1e-5: see the module comment"
    assert worst <= NOISE_GATE


def test_zero_noise_is_exactly_zero():
    meta = nc.rich_metadata()
    pos, tmp, _, _ = _window(1000, 5, seed=8)
    pn, tn = _noise(pos.to(DEV), tmp.to(DEV), meta, 1, 0, noise_std=0.0)
    assert not pn.any() and not tn.any()


# ---- 6: everything downstream of the noise, bit for bit ------------------------------------------------------------------

@pytest.mark.parametrize("w", [2, 5, 16])
@pytest.mark.parametrize("box", [1.0, 25.0])
@pytest.mark.parametrize("batched_targets", [False, True])
def test_sample_equals_the_oracle_on_the_kernels_noise(w, box, batched_targets, monkeypatch):
    n, k, dt = 900, 8, 0.01
    noise_std = NOISE_STD * box
    meta = nc.rich_metadata(box, dt)
    pos, tmp, tp, tt = nc.edge_window(n, w, box, dt, amplitude=2 * noise_std * dt, seed=11 + w)
    if batched_targets:
        tp, tt = tp[None], tt[None]                                           # [1, N, 3] / [1, N, 1]
    seed, draw = SEEDS[1], 5
    pn, tn = _noise(pos.to(DEV), tmp.to(DEV), meta, seed, draw, noise_std=noise_std)
    pn, tn = pn.cpu(), tn.cpu().unsqueeze(-1)
    monkeypatch.setattr(cpu_ref, "position_noise", lambda *a, **kw: pn)
    monkeypatch.setattr(cpu_ref, "temperature_noise", lambda *a, **kw: tn)
    want = cpu_ref.preprocess(pos.clone(), tmp.clone(), meta, tp.clone(), tt.clone(), noise_std, k, dt, box)
    # the inputs do run the wrap code: the remainder, and both signs of the displacement correction
    raw = pos.permute(1, 0, 2) + pn
    assert bool((raw < 0).any()) and bool((raw >= box).any())
    d = (tp.reshape(n, 3) + pn[:, -1]) - want["pos"]
    assert bool((d < -box / 2).any()) and bool((d > box / 2).any())
    tp_dev, tt_dev = tp.to(DEV), tt.to(DEV)
    keep_p, keep_t = tp_dev.clone(), tt_dev.clone()
    got = data_utils.preprocess(pos.to(DEV), tmp.to(DEV), meta, tp_dev, tt_dev, noise_std, k, dt, box,
                                noise_rng="device", noise_seed=seed, noise_draw=draw)
    assert torch.equal(tp_dev, keep_p) and torch.equal(tt_dev, keep_t)        # the caller's targets are not modified
    for name in ("x", "pos", "y_acc", "y_temp_rate"):
        g = getattr(got, name).cpu()
        assert g.shape == want[name].shape, name
        assert torch.equal(g, want[name]), f"{name}: {int((g != want[name]).sum())} of {g.numel()} values differ"
    assert torch.equal(got.edge_index.cpu(), want["edge_index"])
    assert got._cgnn_fixed_k == k and got._cgnn_order.shape == (n,)


# ---- 7: pinned to the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "tiny_k16_box25", "cfg1"])
def test_zero_noise_sample_equals_the_reference_fixture(name):
    g = load_golden(name)
    c, e = torch.from_numpy(g["coords"]), torch.from_numpy(g["energy"])
    meta, w, k = g["metadata"], 5, int(g["k"])
    d = data_utils.preprocess(c[:w].clone(), e[:w].clone(), meta, c[w].clone(), e[w].clone(), 0.0, k, meta["dt"],
                              meta["box_size"], noise_rng="device")
    assert torch.equal(d.x.cpu(), torch.from_numpy(g["x"]))
    assert torch.equal(d.pos.cpu(), torch.from_numpy(g["pos"]))
    assert torch.equal(d.edge_index[0].cpu().to(torch.int32), torch.from_numpy(g["senders"]))
    assert torch.equal(d.y_acc.cpu(), torch.from_numpy(g["y_acc"]))
    assert torch.equal(d.y_temp_rate.cpu(), torch.from_numpy(g["y_temp_rate"]))


# ---- 8: sharding invariance ----------------------------------------------------------------------------------------------

def _sample_args(n, w, seed):
    meta = nc.rich_metadata()
    pos, tmp, tp, tt = _window(n, w, seed)
    return meta, pos.to(DEV), tmp.to(DEV), tp.to(DEV), tt.to(DEV)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_ranks_make_the_one_gpu_sample(world):
    n, k, w = 20_011, 16, 5
    meta, pos, tmp, tp, tt = _sample_args(n, w, seed=31)
    dt, box = meta["dt"], meta["box_size"]
    seed, draw = SEEDS[1], 2 ** 32 + 9
    one = data_utils.preprocess(pos, tmp, meta, tp, tt, NOISE_STD, k, dt, box, noise_rng="device", noise_seed=seed,
                                noise_draw=draw)
    quiet = data_utils.preprocess(pos, tmp, meta, tp, tt, 0.0, k, dt, box, noise_rng="device")
    assert not torch.equal(one.x, quiet.x)                                    # the noise is on
    x = torch.full_like(one.x, float("nan"))
    y_acc, y_tr = torch.full_like(one.y_acc, float("nan")), torch.full_like(one.y_temp_rate, float("nan"))
    owners = torch.zeros(n, dtype=torch.int32, device=DEV)
    senders_one = one.edge_index[0].view(n, k)
    for rank in range(world):
        sh = cdist.sharded_training_sample(pos, tmp, meta, tp, tt, NOISE_STD, k, dt, box, world, rank, seed, draw)
        assert sh.x_feat.shape == (sh.n_owned, one.x.shape[1]) and sh.y_acc.shape == (sh.n_owned, 3)
        assert sh.y_temp_rate.shape == (sh.n_owned, 1)
        x[sh.owned_global], y_acc[sh.owned_global], y_tr[sh.owned_global] = sh.x_feat, sh.y_acc, sh.y_temp_rate
        owners[sh.owned_global] += 1
        table = torch.cat([sh.owned_global, sh.ghost_global])
        assert torch.equal(table[sh.src_local.long()].view(sh.n_owned, k), senders_one[sh.owned_global])
    assert bool((owners == 1).all())                                          # every particle owned exactly once
    assert torch.equal(x, one.x) and torch.equal(y_acc, one.y_acc) and torch.equal(y_tr, one.y_temp_rate)


def test_sharded_step_fed_by_the_sharded_sample_trains_like_one_gpu():
    """One loopback sharded training step (the helpers and gates of tests/test_gpu_sharded_training.py) on shards made
    by sharded_training_sample, against the one-GPU step on preprocess(noise_rng="device")."""
    import test_gpu_sharded_training as st
    world, n, k, d, L, w = 4, 6000, 16, 64, 3, st.W
    snap = synthetic.make_snapshot(n, w, seed=105)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"].to(DEV), snap["InternalEnergy"].to(DEV)
    dt, box, seed, draw = 0.01, 1.0, 99, 3
    g = data_utils.preprocess(c[:w], e[:w], meta, c[w], e[w], NOISE_STD, k, dt, box, noise_rng="device",
                              noise_seed=seed, noise_draw=draw)
    sd = synthetic.make_state_dict(d, d, 2, L, 3, node_in=g.x.shape[1], edge_in=4, seed=106)
    model = st._model(sd, d, L, "fp32")
    want_pred, _, want_grads, want_dx = st._unsharded_step(model, g, dt)
    shards = [cdist.sharded_training_sample(c[:w], e[:w], meta, c[w], e[w], NOISE_STD, k, dt, box, world, r, seed, draw)
              for r in range(world)]
    for r, sh in enumerate(shards):
        cdist.finish_shard(sh, [shards[p].want_global[r] for p in range(world)])
        assert torch.equal(sh.y_acc, g.y_acc[sh.owned_global])
        assert torch.equal(sh.y_temp_rate, g.y_temp_rate[sh.owned_global])
    outs, grads, dx0 = st._loopback_step(model, g, dt, shards)
    for sh, (acc, tr) in zip(shards, outs):
        assert torch.equal(acc, want_pred["acceleration"][sh.owned_global])
        assert torch.equal(tr, want_pred["temp_rate"][sh.owned_global])
    assert set(grads) == set(want_grads)
    assert st._gate_failures(grads, want_grads, st.GTOL) == []
    assert st._err(dx0, want_dx) <= st.GTOL


# ---- 9: statistics on the device -----------------------------------------------------------------------------------------

def test_noise_statistics_at_a_million_particles():
    """The last velocity noise (pos_noise[W-1] - pos_noise[W-2]) / dt is the sum of S independent steps of standard
    deviation noise_std / sqrt(S): its sample standard deviation over 3 N values equals noise_std within
    5 / sqrt(6 N) relative; likewise noise_std x temp_rate_std for the temperature (N values: 5 / sqrt(2 N)).  Two
    draws, and two seeds, correlate below 5 / sqrt(3 N)."""
    n, w = 1_000_000, 6
    meta = nc.rich_metadata()
    dt, trs = meta["dt"], meta["temp_rate_std"]
    pos = torch.rand(w, n, 3, device=DEV)
    tmp = torch.rand(w, n, 1, device=DEV)

    def last_rates(seed, draw):
        pn, tn = _noise(pos, tmp, meta, seed, draw)
        return ((pn[:, -1] - pn[:, -2]).double() / dt).reshape(-1), ((tn[:, -1] - tn[:, -2]).double() / dt).reshape(-1)

    v, r = last_rates(SEEDS[0], 0)
    sv, sr = float(v.std()), float(r.std())
    print(f"velocity noise std / noise_std - 1 = {sv / NOISE_STD - 1:.3e}; rate noise {sr / (NOISE_STD * trs) - 1:.3e}")
    assert abs(sv / NOISE_STD - 1) <= 5 / (6 * n) ** 0.5
    assert abs(sr / (NOISE_STD * trs) - 1) <= 5 / (2 * n) ** 0.5
    assert abs(float(v.mean())) <= 5 * NOISE_STD / (3 * n) ** 0.5
    for what, (v2, _) in (("draw", last_rates(SEEDS[0], 1)), ("seed", last_rates(SEEDS[0] + 1, 0))):
        corr = float(torch.corrcoef(torch.stack([v, v2]))[0, 1])
        print(f"correlation with another {what}: {corr:.3e}")
        assert abs(corr) < 5 / (3 * n) ** 0.5


# ---- 10: determinism and hygiene ---------------------------------------------------------------------------------------

def test_same_seed_and_draw_same_bits_and_no_side_effects():
    n, k, w = 5000, 16, 6
    meta, pos, tmp, tp, tt = _sample_args(n, w, seed=41)
    dt, box = meta["dt"], meta["box_size"]
    keep_p, keep_t = tp.clone(), tt.clone()
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    a = data_utils.preprocess(pos, tmp, meta, tp, tt, NOISE_STD, k, dt, box, noise_rng="device", noise_draw=3)
    b = data_utils.preprocess(pos, tmp, meta, tp, tt, NOISE_STD, k, dt, box, noise_rng="device", noise_seed=1234,
                              noise_draw=3)                                   # None = torch.initial_seed()
    other = data_utils.preprocess(pos, tmp, meta, tp, tt, NOISE_STD, k, dt, box, noise_rng="device", noise_draw=4)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(tp, keep_p) and torch.equal(tt, keep_t)
    for name in ("x", "pos", "y_acc", "y_temp_rate", "edge_index", "edge_attr"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(a.x, other.x)
    # host inputs land on the device with the same result
    h = data_utils.preprocess(pos.cpu(), tmp.cpu(), meta, tp.cpu(), tt.cpu(), NOISE_STD, k, dt, box, device=DEV,
                              noise_rng="device", noise_seed=1234, noise_draw=3)
    assert torch.equal(h.x, a.x) and torch.equal(h.y_acc, a.y_acc) and h.x.is_cuda


def test_device_path_never_synchronises():
    n, k, w = 5000, 16, 6
    meta, pos, tmp, tp, tt = _sample_args(n, w, seed=42)
    dt, box = meta["dt"], meta["box_size"]
    want = data_utils.preprocess(pos, tmp, meta, tp, tt, NOISE_STD, k, dt, box, noise_rng="device", noise_seed=5,
                                 check_bounds=False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = data_utils.preprocess(pos, tmp, meta, tp, tt, NOISE_STD, k, dt, box, noise_rng="device", noise_seed=5,
                                    check_bounds=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got.x, want.x) and torch.equal(got.y_acc, want.y_acc)


def test_c_entry_rejects_bad_arguments_and_launches_nothing():
    n, w = 64, 5
    meta, pos, tmp, tp, tt = _sample_args(n, w, seed=43)
    lib = _lib.load()
    s = _lib.stream_ptr(torch.device(DEV))
    stats = ops.integration_stats(meta)
    x = torch.full((n, 4 * w - 3), 7.0, device=DEV)
    rows = torch.arange(n, device=DEV)

    def call(window=w, n_total=n, rows_ptr=None, n_rows=n, dt=0.01, vel_std=1.0, temp_std=1.0, st=stats, box=1.0):
        return lib.cgnn_training_sample(pos.data_ptr(), tmp.data_ptr(), tp.data_ptr(), tt.data_ptr(), window, n_total,
                                        rows_ptr, n_rows, 3e-4, 1, 0, box, dt, 0.0, vel_std, 0.0, temp_std, st,
                                        x.data_ptr(), None, None, None, None, None, s)

    bad_stats = (C.c_float * 8)(1, 0, 1, 0, 0, 0, 1, 0)                        # acc_std[1] == 0
    zero_trs = (C.c_float * 8)(1, 1, 1, 0, 0, 0, 0, 0)
    for kw in (dict(window=1), dict(n_total=2 ** 31), dict(n_rows=n - 1), dict(dt=0.0), dict(vel_std=0.0),
               dict(temp_std=0.0), dict(st=bad_stats), dict(st=zero_trs), dict(box=0.0), dict(st=None)):
        assert call(**kw) == -1, kw
        assert b"cgnn_training_sample" in lib.cgnn_last_error()
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())                                             # nothing was launched
    assert call(rows_ptr=rows.data_ptr(), n_rows=0) == 0                        # nothing to do
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((x == 7.0).any())
    with pytest.raises(CgnnError):
        ops.training_sample(pos, tmp, meta, 0.01, 1.0, 3e-4, 1, want=("x", "y_acc"))          # target missing
    with pytest.raises(CgnnError):
        ops.training_sample(pos, tmp, meta, 0.01, 1.0, 3e-4, 1, want=("velocity",))
    with pytest.raises(CgnnError):
        ops.training_sample(pos, tmp, meta, 0.01, 1.0, 3e-4, -1, want=("x",))
    with pytest.raises(CgnnError):
        ops.training_sample(pos.cpu(), tmp, meta, 0.01, 1.0, 3e-4, 1, want=("x",))
