"""GPU: the density term of ``training.unrolled_loss`` (``density_loss_weight``, ``density_mesh``, ...): off means the
parent's bits, on means ``losses.density_field_loss`` of every predicted frame added inside the step, with a gradient that
reaches the model through the step's own integration whether or not its outgoing link carries any, in both checkpoint
modes.  The smallest model and window of tests/test_gpu_unrolled_training.py, S in {1, 3}.

Tolerances.  Sums of float32 loss terms: ``(S + 2) 2^-23`` of the sum of the absolute terms.  Gradients that are the same
sum of the same terms added in another order (linearity, the two checkpoint paths): ``GTOL = 2e-5`` of the tensor's largest
entry, what tests/test_gpu_unrolled_checkpoint.py holds its two paths to.  Every distance is printed before it is
asserted.

Measured on an MI355X.  Loss against base + sum of the weighted terms: 6.1e-8 (S = 1, bound 2.6e-5) and 7.0e-6 (S = 3,
bound 2.9e-4), the density terms being 0.3 to 7 times the base loss.  Gradient of base + gradient of the term against the
gradient of both: 1.4e-6 (S = 1), 9.8e-7 (S = 3); ``checkpoint="steps"`` against ``"none"`` with the term on: 2.0e-7."""
import functools

import pytest
import torch

import unroll_checks as uc
from cosmology_gnn_simulation_amd import dist, graph_network, losses, synthetic, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = uc.GTOL
DT = 0.01
N, K, LATENT, ROUNDS, NH, W = 600, 8, 32, 2, 2, 2
# the synthetic frames move by a small fraction of a cell per step, so the density terms are of order 1e-10: a weight
# that brings them to the size of the other terms (tens), so that the sums and the gradients below feel them
MESH, LAMBDA = 8, 1.0e11
BASE = dict(acc_loss_weight=1.0, temp_rate_loss_weight=1.0, momentum_loss_weight=0.1)
TERM_ONLY = dict(acc_loss_weight=0.0, temp_rate_loss_weight=0.0, momentum_loss_weight=0.0)
DENSITY = dict(density_loss_weight=LAMBDA, density_mesh=MESH, density_order=3, density_smoothing=0.1)


@functools.lru_cache(maxsize=None)
def _model():
    m = graph_network.EncodeProcessDecode(LATENT, LATENT, NH, ROUNDS, 3)
    m.load_state_dict(synthetic.make_state_dict(LATENT, LATENT, NH, ROUNDS, 3, node_in=4 * W - 3))
    m = m.to(DEV).train()
    m.message_source, m.train_precision, m.train_edge_messages = "x_j", "fp32", False
    return m


@functools.lru_cache(maxsize=None)
def _data(s):
    snap = synthetic.make_snapshot(N, window=W + s - 1, seed=21)
    c, e = snap["Coordinates"].to(DEV), snap["InternalEnergy"].to(DEV)
    return c[:W], e[:W], c[W:], e[W:]


def _run(s, **kw):
    """-> (UnrolledLoss, {parameter name: gradient on the host, or None})"""
    model = _model()
    model.zero_grad(set_to_none=True)
    out = training.unrolled_loss(model, *_data(s), uc.META, dt=DT, box_size=1.0, num_neighbors=K, **kw)
    out.loss.backward()
    grads = {name: (None if q.grad is None else q.grad.detach().cpu().clone()) for name, q in model.named_parameters()}
    return out, grads


@functools.lru_cache(maxsize=None)
def _runs(s):
    """The calls the tests share, once per S: without the new arguments, with the term, and the term alone"""
    return {"plain": _run(s, **BASE), "both": _run(s, **BASE, **DENSITY), "term": _run(s, **TERM_ONLY, **DENSITY)}


def _distance(what, got, want):
    """Largest ``uc.rel_to_largest`` over the parameters, a ``None`` gradient being ``None`` in both"""
    assert set(got) == set(want)
    worst = 0.0
    for name in want:
        if want[name] is None or got[name] is None:
            assert want[name] is None and got[name] is None, name
            continue
        worst = max(worst, uc.rel_to_largest(got[name], want[name]))
    print(f"{what}: largest gradient distance, of the tensor's largest entry = {worst:.3e}")
    return worst


@pytest.mark.parametrize("s", [1, 3])
def test_weight_zero_is_the_call_without_the_arguments(s):
    want, want_grads = _runs(s)["plain"]
    for kw in (dict(density_loss_weight=0.0), dict(density_loss_weight=0, density_mesh=MESH, density_smoothing=0.1)):
        got, grads = _run(s, **BASE, **kw)
        assert got.density_losses is None and want.density_losses is None
        assert torch.equal(got.loss, want.loss) and torch.equal(got.step_losses, want.step_losses)
        for name in ("Coordinates", "InternalEnergy"):
            assert torch.equal(got.frames[name], want.frames[name])
        for name, g in want_grads.items():
            assert (g is None and grads[name] is None) or torch.equal(grads[name], g), name


@pytest.mark.parametrize("s", [1, 3])
def test_loss_with_the_term_on(s):
    plain, _ = _runs(s)["plain"]
    both, _ = _runs(s)["both"]
    d = both.density_losses
    assert d.dtype == torch.float64 and d.shape == (s,) and not d.requires_grad and both.step_losses.shape == (s, 3)
    assert torch.equal(both.step_losses, plain.step_losses)
    for name in ("Coordinates", "InternalEnergy"):
        assert torch.equal(both.frames[name], plain.frames[name])
    targets = _data(s)[2]                                                      # no noise: the shifted target is the target
    for step in range(s):
        outside = losses.density_field_loss(both.frames["Coordinates"][step], targets[step], 1.0, MESH, 3, 0.1)
        assert float(d[step]) > 0 and torch.equal(d[step], outside)
    added = [LAMBDA * float(v) / s for v in d]                                  # step_weights: 1 / S each
    want = float(plain.loss.detach()) + sum(added)
    scale = float(plain.step_losses.abs().sum()) / s + sum(added)
    err = abs(float(both.loss.detach()) - want)
    print(f"S={s}: loss {float(both.loss.detach()):.6e}, base {float(plain.loss.detach()):.6e}, density terms {added}; error {err:.2e}, "
          f"bound {(s + 2) * 2.0 ** -23 * scale:.2e}")
    assert err <= (s + 2) * 2.0 ** -23 * scale


def test_the_last_steps_integration_carries_the_terms_gradient():
    """S = 1, the density term alone: the only way from the loss to the model is through the integration of the only
    step, whose outgoing link does not exist."""
    out, grads = _run(1, **TERM_ONLY, density_loss_weight=1.0, density_mesh=MESH)
    assert float(out.density_losses[0]) > 0 and float(out.loss) == float(out.density_losses[0].float())
    acc = {name: g for name, g in grads.items() if name.startswith("decoder_acc.")}
    rate = {name: g for name, g in grads.items() if name.startswith("decoder_temp_rate.")}
    assert acc and rate
    for name, g in acc.items():
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, name
    for name, g in rate.items():
        assert g is None or float(g.abs().max()) == 0.0, name


@pytest.mark.parametrize("s", [1, 3])
def test_the_gradient_is_linear_in_the_terms(s):
    runs = _runs(s)
    (_, base), (_, term), (_, both) = runs["plain"], runs["term"], runs["both"]
    added = {}
    for name in both:
        parts = [g for g in (base[name], term[name]) if g is not None]
        added[name] = sum(parts[1:], parts[0]) if parts else None
    assert any(g is not None and float(g.abs().max()) > 0.0 for g in term.values())
    assert _distance(f"S={s} base + term against both", added, both) <= GTOL


def test_checkpointed_steps_give_the_same_bits_and_gradients():
    none, g_none = _runs(3)["both"]
    steps, g_steps = _run(3, **BASE, **DENSITY, checkpoint="steps")
    assert torch.equal(steps.loss, none.loss) and torch.equal(steps.density_losses, none.density_losses)
    assert torch.equal(steps.step_losses, none.step_losses)
    for name in ("Coordinates", "InternalEnergy"):
        assert torch.equal(steps.frames[name], none.frames[name])
    assert _distance("checkpoint='steps' against 'none', term on", g_steps, g_none) <= GTOL


@pytest.mark.parametrize("checkpoint", ["none", "steps"])
def test_cut_links_still_give_every_step_a_gradient(checkpoint):
    """``backprop_steps=0``, the term alone, all weight on one step at a time: the decoder's gradient can only come from
    that step's own integration."""
    for step in range(3):
        weights = [1.0 if t == step else 0.0 for t in range(3)]
        out, grads = _run(3, **TERM_ONLY, **DENSITY, backprop_steps=0, step_weights=weights, checkpoint=checkpoint)
        assert float(out.density_losses[step]) > 0
        for name, g in grads.items():
            if name.startswith("decoder_acc."):
                assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, (step, name)
            if name.startswith("decoder_temp_rate."):
                assert g is None or float(g.abs().max()) == 0.0, (step, name)        # no link, no way through the temperature
    cut, g_cut = _run(3, **BASE, **DENSITY, backprop_steps=0, checkpoint=checkpoint)
    full, g_full = _runs(3)["both"]
    assert torch.equal(cut.loss, full.loss) and torch.equal(cut.density_losses, full.density_losses)    # the same forward
    _distance("backprop_steps=0 against all links (printed only: other gradients)", g_cut, g_full)


def test_batched_and_sharded_losses_do_not_take_the_term_silently():
    p, t, tp, tt = _data(1)
    common = dict(dt=DT, box_size=1.0, num_neighbors=K)
    with pytest.raises((TypeError, NotImplementedError)):
        training.unrolled_batch_loss(_model(), [p], [t], [tp], [tt], uc.META, **common, **DENSITY)
    with pytest.raises((TypeError, NotImplementedError)):
        dist.sharded_unrolled_loss(_model(), p, t, tp, tt, uc.META, **common, **DENSITY)
