"""GPU: activation checkpointing across steps, ``training.unrolled_loss(checkpoint="steps")``, against the plain path
(``checkpoint="none"``) of the same call and against the float64 restatement of tests/unroll_checks.py.

The two paths run the same kernels on the same inputs: loss, step losses and frames are compared with ``torch.equal``.
A gradient is the same sum of the same terms, which autograd may add in another order (a frame's gradient over its
readers, a parameter's over the steps): ``GTOL = 2e-5`` of the tensor's largest entry, the project's gradient tolerance
(``uc.rel_to_largest``); at S = 1 the path is the plain one and the gradients are compared with ``torch.equal``.  Every
distance is printed before it is asserted."""
import functools

import pytest
import torch

import unroll_checks as uc
from cosmology_gnn_simulation_amd import _lib, graph_network, ops, synthetic, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = uc.GTOL
DT = 0.01
N, K, LATENT, ROUNDS, NH = 600, 8, 32, 2, 2
MODES = {"x_j-fp32": ("x_j", "fp32", False), "x_j-fp32x3": ("x_j", "fp32x3", False), "edge-fp32": ("edge", "fp32", True)}
WEIGHTS = (1.0, 1.0, 0.1)       # acc, temp_rate, momentum
CASES = [(3, 1), (6, 2), (2, 3)]
NOISE = dict(noise_std=3e-4, noise_seed=5, noise_draw=1)


def _model(w, source, precision, latent=LATENT, rounds=ROUNDS):
    m = graph_network.EncodeProcessDecode(latent, latent, NH, rounds, 3)
    sd = synthetic.make_state_dict(latent, latent, NH, rounds, 3, node_in=4 * w - 3)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.message_source, m.train_precision = source, precision
    m.train_edge_messages = source == "edge"
    return m, sd


def _data(w, s, n=N, seed=21):
    snap = synthetic.make_snapshot(n, window=w + s - 1, seed=seed)
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    return c[:w], e[:w], c[w:], e[w:]


def _run(model, w, s, min_image, checkpoint, **kw):
    p, t, tp, tt = _data(w, s)
    model.zero_grad(set_to_none=True)
    out = training.unrolled_loss(model, p.to(DEV), t.to(DEV), tp.to(DEV), tt.to(DEV), uc.META, dt=DT, box_size=1.0,
                                 num_neighbors=K, momentum_loss_weight=WEIGHTS[2], min_image_edge_attr=min_image,
                                 checkpoint=checkpoint, **kw)
    out.loss.backward()
    grads = {name: (None if q.grad is None else q.grad.detach().cpu().clone()) for name, q in model.named_parameters()}
    return out, grads


@functools.lru_cache(maxsize=None)
def _pair(mode, w, s):
    """The plain and the checkpointed run of a case, once: (sd, none, grads, steps, grads)."""
    source, precision, min_image = MODES[mode]
    model, sd = _model(w, source, precision)
    none, g_none = _run(model, w, s, min_image, "none", keep_graphs=True)
    steps, g_steps = _run(model, w, s, min_image, "steps", keep_graphs=True)
    return sd, none, g_none, steps, g_steps


def _gradient_distance(what, got, want):
    """Largest ``rel_to_largest`` over the parameters; ``None`` gradients are ``None`` in both."""
    assert set(got) == set(want)
    worst = 0.0
    for name in want:
        if want[name] is None or got[name] is None:
            assert want[name] is None and got[name] is None, name
            continue
        worst = max(worst, uc.rel_to_largest(got[name], want[name]))
    print(f"{what}: largest gradient distance, of the tensor's largest entry = {worst:.3e}")
    return worst


# ---- 1. the same forward bits ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,s", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_checkpointed_forward_gives_the_plain_paths_bits(mode, w, s):
    _, none, _, steps, _ = _pair(mode, w, s)
    assert steps.loss.dtype == torch.float32 and steps.loss.dim() == 0 and steps.loss.grad_fn is not None
    assert torch.equal(steps.loss, none.loss)
    assert steps.step_losses.shape == (s, 3) and not steps.step_losses.requires_grad
    assert torch.equal(steps.step_losses, none.step_losses)
    for name in ("Coordinates", "InternalEnergy"):
        assert steps.frames[name].shape == none.frames[name].shape and not steps.frames[name].requires_grad
        assert torch.equal(steps.frames[name], none.frames[name]), name
    # keep_graphs: detached graphs, the plain path's
    assert len(steps.graphs) == s
    for g, h in zip(steps.graphs, none.graphs):
        assert not g.x.requires_grad and not g.edge_attr.requires_grad
        for name in ("x", "edge_index", "edge_attr", "y_acc", "y_temp_rate", "pos"):
            assert torch.equal(getattr(g, name), getattr(h, name).detach()), name


# ---- 2. the same gradients -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,s", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_checkpointed_gradients_are_the_plain_paths(mode, w, s):
    _, _, g_none, _, g_steps = _pair(mode, w, s)
    edge_params = [name for name in g_none if ".edge_model." in name]
    assert edge_params
    for name in edge_params:        # None under x_j in both; a gradient under edge in both
        assert (g_steps[name] is None) == (g_none[name] is None) == (MODES[mode][0] == "x_j"), name
    assert any(g is not None and float(g.abs().max()) > 0.0 for g in g_steps.values())
    worst = _gradient_distance(f"{mode} W {w} S {s}", g_steps, g_none)
    if s == 1:      # the same path
        for name in g_none:
            assert g_none[name] is None or torch.equal(g_steps[name], g_none[name]), name
    assert worst <= GTOL


# ---- 3. against the yardstick ----------------------------------------------------------------------------------------------

def _restate(sd, source, w, s, graphs, min_image, dtype):
    p, t, tp, tt = _data(w, s)
    sdr = uc.state_dict_of(sd, dtype)
    eis = [g.edge_index.cpu() for g in graphs]
    shifts = [uc.image_shifts(g.edge_attr.detach().cpu(), g.pos.cpu(), ei, 1.0) for g, ei in zip(graphs, eis)] \
        if min_image else None
    out = uc.unrolled(sdr, NH, ROUNDS, source, p, t, tp, tt, uc.META, DT, 1.0, eis, shifts=shifts, weights=WEIGHTS, dtype=dtype)
    out["loss"].backward()
    out["grads"] = {name: q.grad for name, q in sdr.items()}
    return out


def _tensors(loss, step_losses, frames_p, frames_t, grads):
    out = {"loss": loss.detach().reshape(1), "step_losses": step_losses, "InternalEnergy": frames_t.reshape(frames_p.shape[0], -1)}
    out.update({f"grad {name}": g for name, g in grads.items() if g is not None})
    return out, frames_p


def _coords_err(got, want, box=1.0):
    d = uc.wrap(got.detach().cpu().double() - want.detach().cpu().double(), box)      # positions are periodic
    return float(d.abs().max()) / float(want.abs().max())


@pytest.mark.parametrize("mode,w,s", [("edge-fp32", 2, 3), ("x_j-fp32x3", 6, 2)])
def test_checkpointed_loss_and_gradients_match_the_restatement(mode, w, s):
    """The float64-restatement gate of tests/test_gpu_unrolled_training.py on the checkpointed result: every tensor within
    ``max(GTOL, 3 e_ref)`` of the float64 run, ``e_ref`` the float32 restatement's distance to it."""
    source, _, min_image = MODES[mode]
    sd, _, _, out, grads = _pair(mode, w, s)
    assert len(out.graphs) == s and all(uc.valid_knn_lists(g.edge_index, N, K) for g in out.graphs)
    ref = _restate(sd, source, w, s, out.graphs, min_image, torch.float64)
    f32 = _restate(sd, source, w, s, out.graphs, min_image, torch.float32)
    got_t, got_c = _tensors(out.loss, out.step_losses, out.frames["Coordinates"], out.frames["InternalEnergy"], grads)
    ref_t, ref_c = _tensors(ref["loss"], ref["step_losses"], ref["frames_p"], ref["frames_t"], ref["grads"])
    f32_t, f32_c = _tensors(f32["loss"], f32["step_losses"], f32["frames_p"], f32["frames_t"], f32["grads"])
    assert set(got_t) == set(ref_t)
    failures = []
    for name in ref_t:
        e_ref = uc.rel_to_largest(f32_t[name], ref_t[name])
        err, bound = uc.rel_to_largest(got_t[name], ref_t[name]), max(GTOL, 3 * e_ref)
        print(f"{mode} W {w} S {s} steps {name}: HIP error {err:.3e}, e_ref {e_ref:.3e}, bound {bound:.3e}")
        if err > bound:
            failures.append((name, err, bound))
    e_ref_c = _coords_err(f32_c, ref_c)
    err, bound = _coords_err(got_c, ref_c), max(GTOL, 3 * e_ref_c)
    print(f"{mode} W {w} S {s} steps Coordinates: HIP error {err:.3e}, e_ref {e_ref_c:.3e}, bound {bound:.3e}")
    if err > bound:
        failures.append(("Coordinates", err, bound))
    assert not failures, failures


# ---- 4. options ------------------------------------------------------------------------------------------------------------

OPTIONS = {"b=0": dict(backprop_steps=0), "b=1": dict(backprop_steps=1), "b=None": dict(backprop_steps=None),
           "step_weights": dict(step_weights=(0.5, 0.3, 0.2)), "noise": NOISE}


@functools.lru_cache(maxsize=None)
def _option_runs(option):
    w, s = 4, 3
    model, _ = _model(w, "x_j", "fp32")
    return _run(model, w, s, False, "none", **OPTIONS[option]), _run(model, w, s, False, "steps", **OPTIONS[option])


@pytest.mark.parametrize("option", list(OPTIONS))
def test_options_keep_their_meaning_under_checkpointing(option):
    (none, g_none), (steps, g_steps) = _option_runs(option)
    assert torch.equal(steps.loss, none.loss) and torch.equal(steps.step_losses, none.step_losses)
    assert torch.equal(steps.frames["Coordinates"], none.frames["Coordinates"])
    assert torch.equal(steps.frames["InternalEnergy"], none.frames["InternalEnergy"])
    assert _gradient_distance(f"W 4 S 3 {option}", g_steps, g_none) <= GTOL


def test_the_link_gradient_is_not_dropped_under_checkpointing():
    (_, (_, g0)), (_, (_, g_all)) = _option_runs("b=0"), _option_runs("b=None")
    largest = max(uc.rel_to_largest(g0[name], g_all[name]) for name in g_all if g_all[name] is not None)
    print(f"checkpoint='steps': backprop_steps 0 against None, largest gradient distance {largest:.3e}")
    assert largest > 100 * GTOL


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------

def test_two_identical_checkpointed_calls_give_the_same_bits():
    w, s = 3, 2
    model, _ = _model(w, "x_j", "fp32x3")
    a, ga = _run(model, w, s, False, "steps", **NOISE)
    b, gb = _run(model, w, s, False, "steps", **NOISE)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.step_losses, b.step_losses)
    assert torch.equal(a.frames["Coordinates"], b.frames["Coordinates"])
    assert any(g is not None for g in ga.values())
    for name in ga:
        assert (ga[name] is None and gb[name] is None) or torch.equal(ga[name], gb[name]), name


# ---- 6. memory really goes down --------------------------------------------------------------------------------------------

def test_checkpointing_keeps_one_step_of_activations():
    """N = 20 000, k = 8, latent 64, 4 rounds, W = 3: a step keeps about 46 MB of activations, its record is under 2 MB."""
    n, k, w, latent, rounds = 20_000, 8, 3, 64, 4
    model, _ = _model(w, "x_j", "fp32", latent, rounds)
    record = 16 * n + 4 * k * n + 4 * n        # by its definition: a frame, the senders, the order
    assert training.step_record_bytes(n, k) == record
    snap = synthetic.make_snapshot(n, window=w + 3, seed=4)
    c, e = snap["Coordinates"].to(DEV), snap["InternalEnergy"].to(DEV)

    def peak(checkpoint, s):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = training.unrolled_loss(model, c[:w], e[:w], c[w:w + s], e[w:w + s], uc.META, dt=DT, box_size=1.0,
                                     num_neighbors=k, momentum_loss_weight=WEIGHTS[2], checkpoint=checkpoint)
        out.loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.loss))
        del out
        return torch.cuda.max_memory_allocated() - before

    peak("none", 1)         # warm-up: packings and workspaces that stay allocated
    none1, none2, steps4 = peak("none", 1), peak("none", 2), peak("steps", 4)
    print(f"peak above the allocation before the call: none S=1 {none1 / 2**20:.2f} MiB, none S=2 {none2 / 2**20:.2f} MiB, "
          f"steps S=4 {steps4 / 2**20:.2f} MiB; 4 records {4 * record / 2**20:.2f} MiB")
    assert steps4 < none2
    assert steps4 - none1 <= 4 * record + 8 * 2 ** 20


# ---- 7. the guard follows the mode -----------------------------------------------------------------------------------------

def test_memory_guard_follows_the_checkpoint_mode(monkeypatch):
    w, s = 3, 3
    model, _ = _model(w, "x_j", "fp32")
    p, t, tp, tt = (v.to(DEV) for v in _data(w, s))
    shape = (N, K, w, LATENT, LATENT, NH, ROUNDS, s)
    need_none, need_steps = training.unrolled_training_bytes(*shape), training.unrolled_training_bytes(*shape, checkpoint="steps")
    assert need_steps < need_none
    monkeypatch.setattr(training, "free_device_bytes", lambda device: (need_none + need_steps) // 2)
    kw = dict(dt=DT, box_size=1.0, num_neighbors=K)
    real = ops.training_sample
    monkeypatch.setattr(ops, "training_sample", lambda *a, **k_: pytest.fail("launched"))
    with pytest.raises(_lib.CgnnError, match="device memory"):
        training.unrolled_loss(model, p, t, tp, tt, uc.META, checkpoint="none", **kw)
    monkeypatch.setattr(ops, "training_sample", real)
    out = training.unrolled_loss(model, p, t, tp, tt, uc.META, checkpoint="steps", **kw)
    out.loss.backward()
    assert bool(torch.isfinite(out.loss))


# ---- 8. which forward runs -------------------------------------------------------------------------------------------------

def test_frozen_parameters_take_the_inference_forward_in_both_modes():
    """No parameter requires a gradient: ``"steps"`` takes the ``"none"`` path, whose ``model(graph)`` is then the
    inference forward (``node_precision`` kernels), not the training forward a checkpointed step runs."""
    w, s = 3, 2
    model, _ = _model(w, "x_j", "fp32")
    model.node_precision, model.train_precision = "fp16x2", "fp32"
    for q in model.parameters():
        q.requires_grad_(False)
    p, t, tp, tt = (v.to(DEV) for v in _data(w, s))
    kw = dict(dt=DT, box_size=1.0, num_neighbors=K, momentum_loss_weight=WEIGHTS[2], keep_graphs=True)
    none = training.unrolled_loss(model, p, t, tp, tt, uc.META, checkpoint="none", **kw)
    steps = training.unrolled_loss(model, p, t, tp, tt, uc.META, checkpoint="steps", **kw)
    mse = torch.nn.functional.mse_loss
    with torch.no_grad():       # not vacuous: the two forwards differ in their bits on this graph
        inference, train = model(none.graphs[0]), model._forward_train(none.graphs[0])
    differing = int((inference["acceleration"] != train["acceleration"]).sum())
    print(f"inference (fp16x2) against training (fp32) forward on step 0's graph: {differing} of "
          f"{train['acceleration'].numel()} acceleration entries differ")
    assert not torch.equal(inference["acceleration"], train["acceleration"])
    for out in (none, steps):
        assert not out.loss.requires_grad
    assert torch.equal(steps.loss, none.loss) and torch.equal(steps.step_losses, none.step_losses)
    for name in ("Coordinates", "InternalEnergy"):
        assert torch.equal(steps.frames[name], none.frames[name]), name
    for out in (none, steps):
        assert len(out.graphs) == s
        for i, g in enumerate(out.graphs):
            with torch.no_grad():
                pred = model(g)
            assert torch.equal(out.step_losses[i, 0], mse(pred["acceleration"], g.y_acc)), i
