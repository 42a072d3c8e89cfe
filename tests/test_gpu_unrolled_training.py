"""GPU: the multi-step training loss (``training.unrolled_loss``) and its three link kernels
(cgnn_training_sample_backward, cgnn_rollout_integrate_backward, cgnn_edge_attr_backward) against torch autograd of the
plain-torch restatement in tests/unroll_checks.py, run in float64 on the CPU.

Bounds.  A link kernel's output is a sum of at most four float32 terms per entry: ``GTOL = 2e-5`` of the tensor's largest
entry (tests/test_gpu_training.py), expected about 1e-6.  End to end, S = 1 is held to ``GTOL``; for S > 1 the compounded
rounding of S float32 model steps is measured, not derived: ``e_ref`` is the distance of the same restatement run in
float32 on the CPU to its float64 run (per tensor, relative to the largest entry), and the HIP result must lie within
``max(GTOL, 3 e_ref)`` of the float64 run (3: the kernels sum in other orders).  Every figure is printed before it is
asserted.  The link kernels and the Python links are also gated exactly, on problems where float32 does not round and at
every block edge, in tests/test_gpu_unroll_link_gates.py.

Measured on an MI355X.  Link kernels: 1.8e-7 (sample), 1.1e-7 (integrate), 1.8e-7 (edge features).  End to end, the
largest error over loss, step losses, frames and all parameter gradients, HIP error | e_ref of that tensor:
    (W, S)    x_j fp32            x_j fp32x3          edge fp32 (minimum-image features)
    (3, 1)    7.7e-7              1.2e-6              1.6e-6
    (6, 2)    7.9e-6 | 8.8e-6     7.5e-6 | 8.8e-6     4.8e-6 | 4.2e-6
    (2, 3)    2.0e-5 | 2.0e-5     1.9e-5 | 2.0e-5     1.07e-4 | 1.08e-4"""
import functools

import pytest
import torch

import unroll_checks as uc
from cosmology_gnn_simulation_amd import _lib, data_utils, graph_network, losses, ops, synthetic, training
from cosmology_gnn_simulation_amd.one_step import integrate_one_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = uc.GTOL
DT = 0.01
META3 = dict(uc.META, acc_std=[1.1, 0.7, 1.9], acc_mean=[0.01, -0.02, 0.03], temp_rate_std=1.7, temp_rate_mean=0.05)


def _err(got, want, what):
    e = uc.rel_to_largest(got, want)
    print(f"{what}: max |got - want| / max |want| = {e:.3e}")
    return e


def _cfg(meta, box, n):
    return training._LinkConfig(meta, DT, box, n, torch.device(DEV))


# ---- 1. forward bits ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,box", [(2, 1.0), (6, 2.5)])
def test_differentiable_links_give_the_forward_kernels_bits(w, box):
    n, k = 1500, 8
    pos, tmp = uc.crossing_window(n, w, box, seed=w, extra=1)
    pos, tmp = pos.to(DEV), tmp.to(DEV)
    meta = dict(META3, dt=DT, box_size=box)
    cfg = _cfg(meta, box, n)
    frames = [p.clone().requires_grad_(True) for p in pos[:w]] + [t.clone().requires_grad_(True) for t in tmp[:w]]
    got = training._SampleLink.apply(cfg, None, None, pos[w], tmp[w], *frames)
    want = ops.training_sample(pos[:w], tmp[:w], meta, DT, box, 0.0, 0, 0, pos[w], tmp[w])
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:333].to(DEV)
    want_rows = ops.training_sample(pos[:w], tmp[:w], meta, DT, box, 0.0, 0, 0, pos[w], tmp[w], rows)
    for g, name in zip(got, ("x", "recent_pos", "y_acc", "y_temp_rate")):
        assert g.requires_grad and torch.equal(g, want[name]), name
        assert torch.equal(g[rows], want_rows[name]), name
    acc, rate = torch.randn(n, 3, device=DEV), torch.randn(n, 1, device=DEV)
    new_p, new_t, _ = training._IntegrateLink.apply(cfg, None, None, acc.requires_grad_(True), rate, pos[w - 2], pos[w - 1],
                                                    tmp[w - 1])
    want_p, want_t = integrate_one_step(acc.detach(), rate, pos[:w], tmp[:w].unsqueeze(-1), meta)
    assert new_p.requires_grad and torch.equal(new_p, want_p) and torch.equal(new_t.reshape(n, 1), want_t)
    recent = got[1]
    for min_image in (False, True):
        ea, snd = training._KnnEdgeAttr.apply(recent, None, box, k, "uniform", min_image)
        want_snd, want_ea, _ = ops.knn_periodic(recent.detach(), box, k, min_image_edge_attr=min_image)
        assert ea.requires_grad and not snd.requires_grad
        assert torch.equal(ea, want_ea) and torch.equal(snd, want_snd)
    order = training.spatial_order(recent, box)                 # the locality hint: a permutation, cell after cell
    assert order.dtype == torch.int32 and torch.equal(order.long().sort().values, torch.arange(n, device=DEV))
    assert torch.equal(order, training.spatial_order(recent.detach().clone(), box))


def _frame_grads(link, frames, d_outs):
    """The outputs of ``link(*leaves)`` on fresh leaves of ``frames`` and the leaves' gradients for ``d_outs``."""
    leaves = [f.clone().requires_grad_(True) for f in frames]
    outs = link(*leaves)
    return outs, torch.autograd.grad(outs, leaves, d_outs)


@pytest.mark.parametrize("w", [2, 6])
def test_all_rows_and_an_identity_row_list_are_one_link(w):
    """``rows=None`` / ``ids=None`` (whole frames: no row list, no scatter) against the row forms of the same Functions
    on n = 257 rows: one row past a 256-thread block and past four 64-row blocks of the sample backward.  Exact equality
    throughout: the same float32 operations in the same order, followed by an index copy."""
    n, box = 257, 2.5
    pos, tmp = uc.crossing_window(n, w, box, seed=20 + w, extra=1)
    pos, tmp = pos.to(DEV), tmp.to(DEV)
    cfg = _cfg(dict(META3, dt=DT, box_size=box), box, n)
    gen = torch.Generator().manual_seed(w)
    every = torch.arange(n, device=DEV)
    some = torch.randperm(n, generator=gen)[:100].to(DEV)
    rest = torch.ones(n, dtype=torch.bool, device=DEV)
    rest[some] = False
    assert int(rest.sum()) == n - 100

    def sample(rows):
        return lambda *leaves: training._SampleLink.apply(cfg, rows, None, pos[w], tmp[w], *leaves)

    def integrate(ids, acc, rate):
        return lambda p2, p1, t1: training._IntegrateLink.apply(cfg, ids, None, acc, rate, p2, p1, t1)[:2]

    def masked(d_outs):     # the other rows' output gradients set to zero
        return [d.masked_fill(rest.view(-1, *[1] * (d.dim() - 1)), 0.0) for d in d_outs]

    def check_subset(sub, full):    # a subset's frame gradients: the all-rows ones of masked gradients, zero rows exactly zero
        for got, want in zip(sub, full):
            assert torch.equal(got, want)
            assert int(torch.count_nonzero(got[rest])) == 0

    # the sample link: all 2W frames
    frames = list(pos[:w]) + list(tmp[:w])
    d_outs = [torch.randn(shape, generator=gen).to(DEV) for shape in ((n, 4 * w - 3), (n, 3), (n, 3), (n,))]
    outs_all, grads_all = _frame_grads(sample(None), frames, d_outs)
    outs_id, grads_id = _frame_grads(sample(every), frames, d_outs)
    assert len(grads_all) == 2 * w
    for a, b in zip(outs_all + grads_all, outs_id + grads_id):
        assert a.shape == b.shape and torch.equal(a, b)
    outs_sub, grads_sub = _frame_grads(sample(some), frames, [d[some] for d in d_outs])
    for a, b in zip(outs_sub, outs_all):
        assert torch.equal(a, b[some])
    check_subset(grads_sub, _frame_grads(sample(None), frames, masked(d_outs))[1])

    # the integrate link: the frames p2, p1 and t1 (the predictions' gradients are rows on either side)
    acc, rate = torch.randn(n, 3, generator=gen).to(DEV), torch.randn(n, 1, generator=gen).to(DEV)
    last = [pos[w - 2], pos[w - 1], tmp[w - 1]]
    d_new = [torch.randn(n, 3, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)]
    outs_all, grads_all = _frame_grads(integrate(None, acc, rate), last, d_new)
    outs_id, grads_id = _frame_grads(integrate(every, acc, rate), last, d_new)
    for a, b in zip(outs_all + grads_all, outs_id + grads_id):
        assert a.shape == b.shape and torch.equal(a, b)
    outs_sub, grads_sub = _frame_grads(integrate(some, acc[some], rate[some]), last, [d[some] for d in d_new])
    for a, b in zip(outs_sub, outs_all):
        assert torch.equal(a, b[some])
    check_subset(grads_sub, _frame_grads(integrate(None, acc, rate), last, masked(d_new))[1])
    # the predictions' gradients as well, and the packed block both forms return behind the rows
    a_all, a_id = acc.clone().requires_grad_(True), acc.clone().requires_grad_(True)
    r_all, r_id = rate.clone().requires_grad_(True), rate.clone().requires_grad_(True)
    made_all = training._IntegrateLink.apply(cfg, None, None, a_all, r_all, *last)
    made_id = training._IntegrateLink.apply(cfg, every, None, a_id, r_id, *last)
    assert not made_all[2].requires_grad and torch.equal(made_all[2], made_id[2])
    for a, b in zip(torch.autograd.grad(made_all[:2], (a_all, r_all), d_new), torch.autograd.grad(made_id[:2], (a_id, r_id), d_new)):
        assert a.shape == b.shape and torch.equal(a, b)


# ---- 2. cgnn_training_sample_backward -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sample_reference(n, w, box):
    """Autograd of the restatement, float64, once per shape: the four input gradients and, for each, the window
    gradients they give (the map is linear: a combination's reference is the sum)."""
    pos, tmp = uc.crossing_window(n, w, box, seed=100 * w + n, extra=1)
    lo, hi, moved = uc.crossings(pos[:w], box)
    gen = torch.Generator().manual_seed(n + w)
    grads = [torch.randn(n, 4 * w - 3, generator=gen), torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen),
             torch.randn(n, generator=gen)]
    p64, t64 = pos[:w].double().requires_grad_(True), tmp[:w].double().requires_grad_(True)
    outs = uc.sample(p64, t64, pos[w].double(), tmp[w].double(), dict(META3, dt=DT, box_size=box), DT, box)
    parts = [torch.autograd.grad(o, (p64, t64), g.double(), retain_graph=True, allow_unused=True)
             for o, g in zip(outs, grads)]
    parts = [tuple(torch.zeros_like(z) if d is None else d for d, z in zip(p, (p64, t64))) for p in parts]
    return grads, parts, (lo, hi, moved)


@pytest.mark.parametrize("box", [1.0, 2.5])
@pytest.mark.parametrize("w", [2, 6, 11])
@pytest.mark.parametrize("n", [1, 257, 3000])
def test_training_sample_backward_matches_autograd(n, w, box):
    grads, parts, (lo, hi, moved) = _sample_reference(n, w, box)
    print(f"window crossings: {lo} below -box/2, {hi} above box/2, {moved} positions moved by remainder")
    if n >= 257:     # both branches of wrap and the fix-up of remainder are taken (one particle cannot take them all)
        assert lo + hi >= 64 and lo >= 1 and hi >= 1 and moved >= 64
    meta = dict(META3, dt=DT, box_size=box)
    names = ("d_x", "d_recent_pos", "d_y_acc", "d_y_temp_rate")
    dev = [g.to(DEV) for g in grads]
    sentinel = 777.0
    worst = 0.0
    for mask in range(16):
        kw = {name: dev[i] for i, name in enumerate(names) if mask >> i & 1}
        want_p = sum((parts[i][0] for i in range(4) if mask >> i & 1), torch.zeros(w, n, 3, dtype=torch.float64))
        want_t = sum((parts[i][1] for i in range(4) if mask >> i & 1), torch.zeros(w, n, dtype=torch.float64))
        for first in sorted({0, w - 1}):
            out = (torch.full((w, n, 3), sentinel, device=DEV), torch.full((w, n), sentinel, device=DEV))
            d_pos, d_temp = ops.training_sample_backward(w, n, meta, DT, box, first_frame=first, out=out, **kw)
            assert bool((d_pos[:first] == sentinel).all()) and bool((d_temp[:first] == sentinel).all())
            for got, want in ((d_pos[first:], want_p[first:]), (d_temp[first:], want_t[first:])):
                if float(want.abs().max()) == 0.0:
                    assert float(got.abs().max()) == 0.0
                else:
                    worst = max(worst, uc.rel_to_largest(got, want))
    print(f"n {n} w {w} box {box}: largest error over the 16 combinations = {worst:.3e}")
    assert worst <= GTOL
    # a row list: output row i belongs to particle rows[i]; an id outside [0, n) is skipped
    if n > 1:
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:max(2, n // 3)]
        rows_dev = rows.clone()
        rows_dev[1] = -1
        r = rows.numel()
        out = (torch.full((w, r, 3), sentinel, device=DEV), torch.full((w, r), sentinel, device=DEV))
        kw = {name: dev[i][rows.to(DEV)].contiguous() for i, name in enumerate(names)}
        d_pos, d_temp = ops.training_sample_backward(w, r, meta, DT, box, rows=rows_dev.to(DEV), n_total=n, out=out, **kw)
        want_p, want_t = sum(p[0] for p in parts)[:, rows], sum(p[1] for p in parts)[:, rows]
        assert bool((d_pos[:, 1] == sentinel).all()) and bool((d_temp[:, 1] == sentinel).all())
        keep = torch.arange(r) != 1
        e = max(_err(d_pos[:, keep.to(DEV)], want_p[:, keep], "rows d_pos"),
                _err(d_temp[:, keep.to(DEV)], want_t[:, keep], "rows d_temp"))
        assert e <= GTOL


# ---- 3. cgnn_rollout_integrate_backward ---------------------------------------------------------------------------------

@pytest.mark.parametrize("meta", [uc.META, META3], ids=["scalar", "three-component"])
@pytest.mark.parametrize("n", [1, 1000])
def test_rollout_integrate_backward_matches_autograd(meta, n):
    box = 2.5
    meta = dict(meta, dt=DT, box_size=box)
    gen = torch.Generator().manual_seed(n)
    pos, tmp = uc.crossing_window(n, 2, box, seed=n)
    ins = [torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen), pos[0], pos[1], tmp[1]]
    ins64 = [t.double().requires_grad_(True) for t in ins]
    new_p, new_t = uc.integrate(*ins64, meta, DT, box)
    g_p, g_t = torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen)
    names = ("acc_pred", "temp_rate_pred", "p2", "p1", "t1")
    for use_p, use_t in ((True, True), (True, False), (False, True)):
        want = torch.autograd.grad([new_p, new_t], ins64, [g_p.double() * use_p, g_t.double() * use_t], retain_graph=True)
        got = ops.rollout_integrate_backward(g_p.to(DEV) if use_p else None, g_t.to(DEV) if use_t else None, meta)
        for name, w_ in zip(names, want):
            if float(w_.abs().max()) == 0.0:
                assert float(got[name].abs().max()) == 0.0, name
            else:
                assert _err(got[name].reshape(w_.shape), w_, f"{name} (pos {use_p}, temp {use_t})") <= GTOL
    only = ops.rollout_integrate_backward(g_p.to(DEV), g_t.to(DEV), meta, want=("p1",))        # a subset of the outputs
    assert list(only) == ["p1"]
    assert torch.equal(only["p1"], ops.rollout_integrate_backward(g_p.to(DEV), g_t.to(DEV), meta)["p1"])


# ---- 4. cgnn_edge_attr_backward -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_image", [False, True])
@pytest.mark.parametrize("k", [4, 16])
def test_edge_attr_backward_matches_autograd_and_repeats(k, min_image):
    n, box = 500, 1.0
    gen = torch.Generator().manual_seed(k)
    pos = torch.rand(n, 3, generator=gen) * box
    for axis in range(3):       # a particle within 1e-3 of each face
        pos[2 * axis, axis] = 5e-4
        pos[2 * axis + 1, axis] = box - 5e-4
    snd, ea, _ = ops.knn_periodic(pos.to(DEV), box, k, min_image_edge_attr=min_image)
    ei = torch.stack([snd.long().cpu(), torch.arange(n).repeat_interleave(k)])
    raw = pos[ei[0]] - pos[ei[1]]
    crossing = int((raw.abs() > box / 2).any(-1).sum())
    print(f"{crossing} of {n * k} edges cross a face")
    assert crossing >= 6
    shift = uc.image_shifts(ea.cpu(), pos, ei, box) if min_image else None
    assert (shift is None) or int((shift != 0).any(-1).sum()) == crossing
    p64 = pos.double().requires_grad_(True)
    ref = uc.edge_features(p64, ei, shift)
    assert uc.rel_to_largest(ea, ref) <= 1e-6
    d_ea = torch.randn(n * k, 4, generator=gen)
    want, = torch.autograd.grad(ref, p64, d_ea.double())
    csr = ops.SenderCsr(snd, None, n)
    got = ops.edge_attr_backward(d_ea.to(DEV), ea, snd, k, csr)
    assert bool(torch.isfinite(got).all())
    assert _err(got, want, f"k {k} min_image {min_image}") <= GTOL
    again = ops.edge_attr_backward(d_ea.to(DEV), ea, snd, k, ops.SenderCsr(snd, None, n))
    assert torch.equal(got, again)
    # the self edges (the first of every receiver, length 0): a finite, zero contribution
    assert bool((ea.view(n, k, 4)[:, 0] == 0).all())
    only_self = torch.zeros(n, k, 4)
    only_self[:, 0] = torch.randn(n, 4, generator=gen)
    zero = ops.edge_attr_backward(only_self.view(n * k, 4).to(DEV), ea, snd, k, csr)
    assert torch.equal(zero, torch.zeros_like(zero))


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------

N, K, LATENT, ROUNDS, NH = 600, 8, 32, 2, 2
MODES = {"x_j-fp32": ("x_j", "fp32", False), "x_j-fp32x3": ("x_j", "fp32x3", False), "edge-fp32": ("edge", "fp32", True)}
WEIGHTS = (1.0, 1.0, 0.1)       # acc, temp_rate, momentum


def _model(w, source, precision):
    m = graph_network.EncodeProcessDecode(LATENT, LATENT, NH, ROUNDS, 3)
    sd = synthetic.make_state_dict(LATENT, LATENT, NH, ROUNDS, 3, node_in=4 * w - 3)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.message_source, m.train_precision = source, precision
    m.train_edge_messages = source == "edge"
    return m, sd


def _data(w, s, seed=21):
    snap = synthetic.make_snapshot(N, window=w + s - 1, seed=seed)
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    return c[:w], e[:w], c[w:], e[w:]


def _run_hip(model, w, s, min_image, **kw):
    p, t, tp, tt = _data(w, s)
    model.zero_grad(set_to_none=True)
    out = training.unrolled_loss(model, p.to(DEV), t.to(DEV), tp.to(DEV), tt.to(DEV), uc.META, dt=DT, box_size=1.0,
                                 num_neighbors=K, momentum_loss_weight=WEIGHTS[2], min_image_edge_attr=min_image,
                                 keep_graphs=True, **kw)
    out.loss.backward()
    grads = {name: (None if q.grad is None else q.grad.detach().cpu().clone()) for name, q in model.named_parameters()}
    return out, grads


def _restate(sd, source, w, s, graphs, min_image, dtype, **kw):
    p, t, tp, tt = _data(w, s)
    sdr = uc.state_dict_of(sd, dtype)
    eis = [g.edge_index.cpu() for g in graphs]
    shifts = [uc.image_shifts(g.edge_attr.detach().cpu(), g.pos.cpu(), ei, 1.0) for g, ei in zip(graphs, eis)] \
        if min_image else None
    out = uc.unrolled(sdr, NH, ROUNDS, source, p, t, tp, tt, uc.META, DT, 1.0, eis, shifts=shifts, weights=WEIGHTS,
                      dtype=dtype, **kw)
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


@pytest.mark.parametrize("w,s", [(3, 1), (6, 2), (2, 3)])
@pytest.mark.parametrize("mode", list(MODES))
def test_unrolled_loss_and_gradients_match_the_restatement(mode, w, s):
    """HIP error and e_ref per case: the module docstring and DESIGN.md, "Multi-step training"."""
    source, precision, min_image = MODES[mode]
    model, sd = _model(w, source, precision)
    out, grads = _run_hip(model, w, s, min_image)
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0 and out.loss.grad_fn is not None
    assert out.step_losses.shape == (s, 3) and not out.step_losses.requires_grad
    assert out.frames["Coordinates"].shape == (s, N, 3) and out.frames["InternalEnergy"].shape == (s, N, 1)
    assert len(out.graphs) == s and all(uc.valid_knn_lists(g.edge_index, N, K) for g in out.graphs)
    ref = _restate(sd, source, w, s, out.graphs, min_image, torch.float64)
    got_t, got_c = _tensors(out.loss, out.step_losses, out.frames["Coordinates"], out.frames["InternalEnergy"], grads)
    ref_t, ref_c = _tensors(ref["loss"], ref["step_losses"], ref["frames_p"], ref["frames_t"], ref["grads"])
    e_ref = dict.fromkeys(ref_t, 0.0)
    e_ref_c = 0.0
    if s > 1:
        f32 = _restate(sd, source, w, s, out.graphs, min_image, torch.float32)
        f32_t, f32_c = _tensors(f32["loss"], f32["step_losses"], f32["frames_p"], f32["frames_t"], f32["grads"])
        e_ref = {name: uc.rel_to_largest(f32_t[name], ref_t[name]) for name in ref_t}
        e_ref_c = _coords_err(f32_c, ref_c)
    edge_params = [name for name in grads if ".edge_model." in name]
    assert edge_params
    for name in edge_params:
        if source == "x_j":
            assert grads[name] is None and ref["grads"][name] is None, name
        else:
            assert grads[name] is not None and float(grads[name].abs().max()) > 0.0, name
    assert set(got_t) == set(ref_t)
    failures = []
    worst = (0.0, 0.0)
    for name in ref_t:
        err, bound = uc.rel_to_largest(got_t[name], ref_t[name]), max(GTOL, 3 * e_ref[name])
        print(f"{mode} W {w} S {s} {name}: HIP error {err:.3e}, e_ref {e_ref[name]:.3e}, bound {bound:.3e}")
        worst = max(worst, (err, e_ref[name]))
        if err > bound:
            failures.append((name, err, bound))
    err, bound = _coords_err(got_c, ref_c), max(GTOL, 3 * e_ref_c)
    print(f"{mode} W {w} S {s} Coordinates: HIP error {err:.3e}, e_ref {e_ref_c:.3e}, bound {bound:.3e}")
    print(f"{mode} W {w} S {s} SUMMARY: largest HIP error {max(worst[0], err):.3e} (e_ref of that tensor {worst[1]:.3e})")
    if err > bound:
        failures.append(("Coordinates", err, bound))
    assert not failures, failures


# ---- 6. S = 1 is today's one-step path -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["x_j-fp32", "edge-fp32"])
def test_one_unrolled_step_is_the_one_step_path(mode):
    source, precision, min_image = MODES[mode]
    w = 5
    model, _ = _model(w, source, precision)
    noise = dict(noise_std=3e-4, noise_seed=77, noise_draw=3)
    out, grads = _run_hip(model, w, 1, min_image, **noise)
    p, t, tp, tt = _data(w, 1)
    g = data_utils.preprocess(p.to(DEV), t.to(DEV), uc.META, tp[0].to(DEV), tt[0].to(DEV), noise["noise_std"], K, DT, 1.0,
                              check_bounds=False, noise_rng="device", noise_seed=77, noise_draw=3,
                              min_image_edge_attr=min_image)
    mine = out.graphs[0]
    for name in ("x", "y_acc", "y_temp_rate", "pos", "edge_attr", "edge_index"):
        assert torch.equal(getattr(mine, name).detach(), getattr(g, name)), name
    model.zero_grad(set_to_none=True)
    pred = model(g)
    mse = torch.nn.functional.mse_loss
    loss = (mse(pred["acceleration"], g.y_acc) + mse(pred["temp_rate"], g.y_temp_rate)
            + losses.momentum_conservation_loss(pred["acceleration"], g, DT, WEIGHTS[2]))
    loss.backward()
    assert _err(out.loss, loss, "loss") <= GTOL
    for name, q in model.named_parameters():
        if q.grad is None:
            assert grads[name] is None, name
        else:
            assert _err(grads[name], q.grad, name) <= GTOL, name


# ---- 7. backprop_steps ------------------------------------------------------------------------------------------------------

def test_backprop_steps_zero_is_three_detached_steps_and_all_links_differ():
    w, s = 4, 3
    model, _ = _model(w, "x_j", "fp32")
    out0, g0 = _run_hip(model, w, s, False, backprop_steps=0)
    out_all, g_all = _run_hip(model, w, s, False)
    assert _err(out0.loss, out_all.loss, "loss, b = 0 against b = None") <= 1e-6       # the forward does not depend on b
    assert torch.equal(out0.frames["Coordinates"], out_all.frames["Coordinates"])
    p, t, tp, tt = (v.to(DEV) for v in _data(w, s))
    pos = torch.cat([p, out0.frames["Coordinates"]])
    tmp = torch.cat([t, out0.frames["InternalEnergy"]])
    model.zero_grad(set_to_none=True)
    mse = torch.nn.functional.mse_loss
    for i in range(s):
        g = data_utils.preprocess(pos[i:i + w], tmp[i:i + w], uc.META, tp[i], tt[i], 0.0, K, DT, 1.0, check_bounds=False,
                                  noise_rng="device", noise_seed=1)
        pred = model(g)
        loss = (mse(pred["acceleration"], g.y_acc) + mse(pred["temp_rate"], g.y_temp_rate)
                + losses.momentum_conservation_loss(pred["acceleration"], g, DT, WEIGHTS[2]))
        (loss / s).backward()
    largest = 0.0
    for name, q in model.named_parameters():
        if q.grad is None:
            assert g0[name] is None and g_all[name] is None
            continue
        assert _err(g0[name], q.grad, f"b = 0, {name}") <= GTOL, name
        largest = max(largest, _err(g_all[name], q.grad, f"b = None, {name}"))
    assert largest > 100 * GTOL      # the gradient through the links is not silently zero
    _, g2 = _run_hip(model, w, s, False, backprop_steps=2)
    _, g9 = _run_hip(model, w, s, False, backprop_steps=9)
    for name in g_all:       # b >= S - 1 is every link
        if g_all[name] is not None:
            assert uc.rel_to_largest(g2[name], g_all[name]) <= GTOL and uc.rel_to_largest(g9[name], g_all[name]) <= GTOL, name
    _, g1 = _run_hip(model, w, s, False, backprop_steps=1)      # one link: neither none nor all of them
    assert any(g1[name] is not None and uc.rel_to_largest(g1[name], g_all[name]) > 100 * GTOL
               and uc.rel_to_largest(g1[name], g0[name]) > 100 * GTOL for name in g_all)


# ---- 8. reproducibility -------------------------------------------------------------------------------------------------------

def test_two_identical_calls_give_the_same_bits():
    w, s = 3, 2
    model, _ = _model(w, "x_j", "fp32x3")
    a, ga = _run_hip(model, w, s, False, noise_std=3e-4, noise_seed=5, noise_draw=1)
    b, gb = _run_hip(model, w, s, False, noise_std=3e-4, noise_seed=5, noise_draw=1)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.step_losses, b.step_losses)
    assert torch.equal(a.frames["Coordinates"], b.frames["Coordinates"])
    for name in ga:
        assert (ga[name] is None and gb[name] is None) or torch.equal(ga[name], gb[name]), name
    c, _ = _run_hip(model, w, s, False, noise_std=3e-4, noise_seed=5, noise_draw=2)
    assert not torch.equal(a.loss, c.loss)


# ---- 9. the C ABI rejects bad arguments and launches nothing -------------------------------------------------------------

def test_link_entries_reject_bad_arguments_and_launch_nothing():
    lib = _lib.load()
    s = _lib.stream_ptr(torch.device(DEV))
    w, n, k = 4, 8, 2
    stats = ops.integration_stats(synthetic.make_metadata())
    bad_stats = ops.integration_stats(dict(synthetic.make_metadata(), acc_std=0.0))
    d_x = torch.ones(n, 4 * w - 3, device=DEV)
    d_y = torch.ones(n, 3, device=DEV)
    d_pos, d_temp = torch.zeros(w, n, 3, device=DEV), torch.zeros(w, n, device=DEV)
    rows = torch.arange(n, dtype=torch.int64, device=DEV)

    def sample(window=w, n_total=n, rows_=None, n_rows=n, first=0, box=1.0, dt=DT, vel_std=1.0, temp_std=1.0, st=stats,
               dp=d_pos.data_ptr(), dy=d_y.data_ptr()):
        return lib.cgnn_training_sample_backward(d_x.data_ptr(), None, dy, None, window, n_total, rows_, n_rows, first, box,
                                                 dt, vel_std, temp_std, st, dp, d_temp.data_ptr(), s)
    assert sample(window=1) == -1 and sample(window=33) == -1
    assert sample(first=-1) == -1 and sample(first=w) == -1
    assert sample(n_rows=n - 1) == -1                           # no row list, not all rows
    assert sample(n_total=2 ** 31, rows_=rows.data_ptr()) == -1
    assert sample(box=0.0) == -1 and sample(dt=0.0) == -1 and sample(vel_std=0.0) == -1 and sample(temp_std=0.0) == -1
    assert sample(st=None) == -1 and sample(st=bad_stats) == -1  # target gradients need the statistics
    assert sample(dp=None) == -1
    assert b"cgnn_training_sample_backward" in lib.cgnn_last_error()
    g3, g1 = torch.ones(n, 3, device=DEV), torch.ones(n, device=DEV)
    outs = [torch.zeros(n, 3, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, 3, device=DEV),
            torch.zeros(n, 3, device=DEV), torch.zeros(n, device=DEV)]

    def integ(n_rows=n, st=stats, dt=DT, box=1.0, ptrs=None):
        ptrs = [o.data_ptr() for o in outs] if ptrs is None else ptrs
        return lib.cgnn_rollout_integrate_backward(g3.data_ptr(), g1.data_ptr(), n_rows, st, dt, box, *ptrs, s)
    assert integ(n_rows=-1) == -1 and integ(st=None) == -1 and integ(dt=0.0) == -1 and integ(box=-1.0) == -1
    assert integ(ptrs=[None] * 5) == -1
    assert b"cgnn_rollout_integrate_backward" in lib.cgnn_last_error()
    ea = torch.ones(n * k, 4, device=DEV)
    snd = torch.zeros(n * k, dtype=torch.int32, device=DEV)
    csr = ops.SenderCsr(snd, None, n)
    d_node = torch.zeros(n, 3, device=DEV)

    def edge(n_=n, k_=k, dea=ea.data_ptr(), ea_=ea.data_ptr(), snd_=snd.data_ptr(), rp=csr.row_ptr.data_ptr(),
             col=csr.col.data_ptr(), out=d_node.data_ptr()):
        return lib.cgnn_edge_attr_backward(dea, ea_, snd_, n_, k_, rp, col, out, s)
    assert edge(n_=-1) == -1 and edge(k_=0) == -1 and edge(n_=2 ** 30, k_=4) == -1
    assert edge(dea=None) == -1 and edge(ea_=None) == -1 and edge(snd_=None) == -1 and edge(rp=None) == -1
    assert edge(col=None) == -1 and edge(out=None) == -1
    assert edge(ea_=ea.data_ptr() + 4) == -1                    # the float4 reads need 16-byte alignment
    assert b"cgnn_edge_attr_backward" in lib.cgnn_last_error()
    torch.cuda.synchronize()
    for t_ in [d_pos, d_temp, d_node] + outs:
        assert torch.equal(t_, torch.zeros_like(t_))
    # empty problems are fine and launch nothing either
    assert lib.cgnn_rollout_integrate_backward(None, None, 0, stats, DT, 1.0, *[o.data_ptr() for o in outs], s) == 0
    assert edge(n_=0) == 0


def test_memory_guard_refuses_before_any_launch(monkeypatch):
    model, _ = _model(3, "x_j", "fp32")
    p, t, tp, tt = _data(3, 2)
    monkeypatch.setattr(training, "free_device_bytes", lambda device: 1024)
    monkeypatch.setattr(ops, "training_sample", lambda *a, **kw: pytest.fail("launched"))
    with pytest.raises(_lib.CgnnError, match="device memory"):
        training.unrolled_loss(model, p.to(DEV), t.to(DEV), tp.to(DEV), tt.to(DEV), uc.META, dt=DT, box_size=1.0,
                               num_neighbors=K)
