"""GPU: training under message_source="edge" (model.train_edge_messages = True) -- the HIP backward of the edge stream
(cgnn_edge_mlp_backward, cgnn_linear2_rows and the fixed-order reductions) against torch autograd on the CPU oracle.

Gates are those of test_gpu_training.py: outputs 1e-5; gradients 2e-5 of each tensor's largest entry, 1.5x that at
latent 256 (every dot product twice as long)."""
import pytest
import torch

import backward_checks as bc
from backward_checks import GTOL, Lin as _Lin, close as _close, edge_sd as _edge_sd, edges as _edges
from cosmology_gnn_simulation_amd import _lib, data_utils, graph_network, losses, ops, synthetic, training
from cosmology_gnn_simulation_amd.graph import Batch, Data
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


_PAIRS = [(32, 32), (64, 64), (128, 128), (256, 256), (128, 64), (128, 256)]      # (hidden, latent)


@pytest.mark.parametrize("graph", ["k8", "k16", "k32", "general"])
@pytest.mark.parametrize("pair_i", range(len(_PAIRS)))
@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "fp32x3 with the forward recomputed on fp16x2"])
def test_edge_mlp_backward_matches_autograd(pair_i, precision, graph):
    """ops.edge_mlp_backward + the reductions of one round (training.edge_round_grads, linear2_rows) against torch autograd
    of L = <e + u, de_next> + <agg(u), d_agg>, u = mlp_ln(cat[x[src], x[dst], e]): de, every weight / bias / LayerNorm
    gradient, dPs / dPd and dx.  Every (hidden, latent) pair, 1..3 hidden layers (cycled), the three arithmetic pairings,
    E not a multiple of 32, fixed in-degree 8 / 16 / 32 and a general edge list.  Besides the 2e-5 of each tensor's
    largest entry, EVERY row of de, dPs, dPd and dx is held to 2e-5 of its own norm against float64 autograd
    (backward_checks.py).  For that gate the edges are margin-filtered: an edge with a ReLU input at rounding distance from
    zero (min |a| / max |a| <= 1e-5 over a hidden layer) has a discontinuous gradient that any f32 evaluation may get wrong
    by 1 / sqrt(H), so its e row is re-drawn from the same generator (most seeds have none).  All sizes here run one tile
    per wave; test_gpu_backward_gates.py runs more."""
    H, D = _PAIRS[pair_i]
    nh = 1 + (pair_i + len(graph)) % 3
    gen = torch.Generator().manual_seed(17 * pair_i + len(graph) + len(precision))
    n = 37 if graph != "k32" else 29      # 296, 592, 188 edges (ragged last tile); 928 at k = 32 (whole tiles)
    src, dst, fixed_k = _edges(gen, n, graph)
    ne = src.numel()
    sd = _edge_sd(gen, D, H, nh)
    x = torch.randn(n, D, generator=gen)
    e = torch.randn(ne, D, generator=gen)
    de_next = torch.randn(ne, D, generator=gen)
    d_agg = torch.randn(n, D, generator=gen)
    bc.redraw_fragile_edge_rows(gen, sd, x, src, dst, e, nh, cap=None)
    want64 = bc.edge_reference(dict(sd=sd, x=x, e=e, src=src, dst=dst, de_next=de_next, d_agg=d_agg, n=n, ne=ne, H=H, D=D, nh=nh))
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    x.requires_grad_(True)
    e.requires_grad_(True)
    u = cpu_ref.mlp_ln(sd, "m", torch.cat([x[src.long()], x[dst.long()], e], dim=-1), nh)
    agg = torch.zeros(n, D).index_add(0, dst.long(), u)
    ((e + u) * de_next).sum().add((agg * d_agg).sum()).backward()

    lins = [_Lin(sd[f"m.0.{2 * i}.weight"].detach().to(DEV), sd[f"m.0.{2 * i}.bias"].detach().to(DEV)) for i in range(nh + 1)]
    lnm = _Lin(sd["m.1.weight"].detach().to(DEV), sd["m.1.bias"].detach().to(DEV))
    prec = precision.split()[0]
    te = training._TrainEdge(lins, lnm, D, prec)
    if prec == "fp32x3":      # the (fp32x3, fp32x3) or the (fp16x2, fp32x3) pairing at every shape
        wb = [(l.weight, l.bias) for l in lins]
        rec = "fp16x2" if precision.endswith("fp16x2") else "fp32x3"
        te.rec = ops.PackedMLP(wb, (lnm.weight, lnm.bias), rec, first_layer_cols=(2 * D, D))
    assert (te.rec.precision == _lib.F16X2) == precision.endswith("fp16x2")
    xd, srcd, dstd = x.detach().to(DEV), src.to(DEV), dst.to(DEV)
    ps, pd = ops.project_nodes(te.ws, te.wd, xd, p_format=_lib.P_F32)
    et = ops.TiledRows.from_rows(e.detach().to(DEV))
    de = ops.TiledRows.from_rows(de_next.to(DEV))
    scratch = ops.BackwardScratch(ne, H, D, nh, DEV)
    dy = torch.empty(ne, D, device=DEV)
    by_sender = ops.SenderCsr(srcd, None, n)
    by_receiver = ops.SenderCsr(dstd, None, n) if fixed_k == 0 else None
    de_sep = de.empty_like()
    ops.edge_mlp_backward(te.rec, te.bwd, ps, pd, srcd, dstd, et, d_agg.to(DEV), de, scratch, dy, de_sep)
    dy_first = dy.clone()
    grads, dps, dpd = training.edge_round_grads(te, scratch, dy, et, xd, dstd, fixed_k, by_sender, by_receiver)
    dx = ops.linear2_rows(te.wst, te.wdt, dps, dpd)
    assert _close(dy_first, de_next + d_agg[dst.long()], 1e-6)
    assert _close(de_sep.to_rows(), e.grad)
    assert _close(dx, x.grad)
    for name, got in (("de", de_sep.to_rows()), ("dps", dps), ("dpd", dpd), ("dx", dx)):
        bc.assert_rows(got, want64[name], name)
    names = [f"m.0.{2 * i}.{p}" for i in range(nh + 1) for p in ("weight", "bias")] + ["m.1.weight", "m.1.bias"]
    gtol = GTOL if D <= 128 else 1.5 * GTOL
    for name, g in zip(names, grads, strict=True):
        assert g.shape == sd[name].shape, name
        assert _close(g, sd[name].grad, gtol), name
    # dPs / dPd: the sender / receiver sums of dL/dh1 (dh1 = grad of the first Linear's output, from autograd)
    h1 = torch.cat([x[src.long()], x[dst.long()], e], dim=-1).detach() @ sd["m.0.0.weight"].detach().t() + sd["m.0.0.bias"].detach()
    h1.requires_grad_(True)
    z = h1.relu()
    for i in range(1, nh + 1):
        z = z @ sd[f"m.0.{2 * i}.weight"].detach().t() + sd[f"m.0.{2 * i}.bias"].detach()
        if i < nh:
            z = z.relu()
    z = torch.nn.functional.layer_norm(z, (D,), sd["m.1.weight"].detach(), sd["m.1.bias"].detach())
    (z * (de_next + d_agg[dst.long()])).sum().backward()
    assert _close(dps, torch.zeros(n, H, dtype=torch.float64).index_add(0, src.long(), h1.grad.double()))
    assert _close(dpd, torch.zeros(n, H, dtype=torch.float64).index_add(0, dst.long(), h1.grad.double()))
    # in place (de_out = de_in), and d e written in rows (what the edge encoder's backward reads): the same bits
    ops.edge_mlp_backward(te.rec, te.bwd, ps, pd, srcd, dstd, et, d_agg.to(DEV), de, scratch, dy, de.buf, de_out_rows=True)
    assert torch.equal(de.buf[:ne], de_sep.to_rows())


def _problem(n, k, latent, nh, steps, seed, window=5):
    snap = synthetic.make_snapshot(n, window, seed=seed)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    dt = 0.01
    g = data_utils.preprocess(c[:window].clone(), e[:window].clone(), meta, c[window].clone(), e[window].clone(), 0.0, k,
                              dt, 1.0)
    sd = synthetic.make_state_dict(latent, latent, nh, steps, 3, node_in=g.x.shape[1], edge_in=4, seed=seed + 1)
    return g, sd, dt


def _reference(sd, g, nh, steps, dt, batch=None, num_graphs=1, dtype=torch.float32):
    """Autograd of the oracle under message_source="edge" with the loss of test_gpu_training._reference_grads (evaluated in
    ``dtype``)."""
    sdr = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = g.x.detach().cpu().to(dtype).clone().requires_grad_(True)
    ea = g.edge_attr.detach().cpu().to(dtype).clone().requires_grad_(True)
    out = cpu_ref.encode_process_decode(sdr, x, g.edge_index.cpu().long(), ea, nh, steps, message_source="edge")
    mse = torch.nn.functional.mse_loss
    b = torch.zeros(x.shape[0], dtype=torch.long) if batch is None else batch.cpu().long()
    loss = (mse(out["acceleration"], g.y_acc.cpu().to(dtype)) + 0.5 * mse(out["temp_rate"], g.y_temp_rate.cpu().to(dtype))
            + cpu_ref.momentum_conservation_loss(out["acceleration"], b, num_graphs, dt, 0.1))
    loss.backward()
    return loss.detach(), sdr, x.grad, ea.grad, out


def _edge_model(latent, nh, steps, sd, train_precision="fp32", locality=True):
    model = graph_network.EncodeProcessDecode(latent, latent, nh, steps, 3)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    model.message_source = "edge"
    model.train_edge_messages = True
    model.train_precision = train_precision
    model.locality_sort = locality
    return model


def _loss(pred, g, dt, w_tr=0.5):
    mse = torch.nn.functional.mse_loss
    return (mse(pred["acceleration"], g.y_acc) + w_tr * mse(pred["temp_rate"], g.y_temp_rate)
            + losses.momentum_conservation_loss(pred["acceleration"], g, dt, 0.1))


# At the shapes with latent >= 128 the step's gradients are ill-conditioned under any f32 evaluation: a ReLU input or a
# LayerNorm term that lands near zero on one of 24k (16k) edges takes a different branch under a different rounding, and
# that edge's error spreads through the later rounds.  Measured distance from float64 autograd of the oracle, as max |err| /
# max |grad| (parameters / g.x.grad / d edge_attr):
#   (1500, 16, 128, 2, 3)  torch float32, oracle order 3.2e-5 / 1.6e-3 / 2.5e-2;  HIP fp32 1.4e-4 / 2.1e-2 / 2.6e-2;
#                          HIP fp32x3 1.3e-6 / 5.1e-7 / 7.5e-7;  a float32 CPU evaluation in the engine's first-layer order
#                          (Ps[src] + Pd[dst] + e We^T) 1.0e-6 / 5.2e-7 / 8.3e-7 in one run, 3.2e-4 / 3.0e-2 / - in another
#                          evaluation of that order (a different CPU summation)
#   (500, 32, 256, 2, 2)   torch float32 1.3e-4 / 1.6e-3 / 3.5e-2;  HIP fp32 1.3e-4 / 1.6e-3 / 3.5e-2 (the same branch as
#                          torch);  HIP fp32x3 1.3e-4 / 7.4e-4 / 1.6e-2;  engine-order CPU float32 4.2e-5 / 3.1e-4 / 1.9e-2
# so no f32 implementation meets 2e-5 there.  Those shapes are gated against float64 autograd at ILL_PTOL (parameters) and
# ILL_XTOL (g.x.grad, d edge_attr), about twice the worst f32 evaluation measured; their outputs keep the 1e-5 gate.
ILL_PTOL, ILL_XTOL = 5e-4, 6e-2


@pytest.mark.parametrize("n,k,latent,nh,steps", [(600, 8, 32, 2, 2), (1500, 16, 128, 2, 3), (900, 8, 64, 1, 4),
                                                  (500, 32, 256, 2, 2)])
@pytest.mark.parametrize("locality", [True, False])
@pytest.mark.parametrize("train_precision", ["fp32", "fp32x3"])
def test_edge_mode_training_gradients_match_reference_autograd(n, k, latent, nh, steps, locality, train_precision):
    """Every parameter -- encoder.edge_model.* and processor.*.edge_model.* included, non-None on both sides --, g.x.grad
    and d edge_attr against autograd of cpu_ref.encode_process_decode(..., message_source="edge"): the float32 oracle at
    2e-5 of each tensor's largest entry where the problem is well conditioned, float64 at ILL_PTOL / ILL_XTOL at latent
    >= 128 (see above).  Outputs and loss within 1e-5 of the float32 oracle at every shape."""
    g, sd, dt = _problem(n, k, latent, nh, steps, seed=n)
    want_loss, sdr, want_dx, want_dea, want_out = _reference(sd, g, nh, steps, dt)
    ill = latent >= 128
    if ill:
        _, sdr, want_dx, want_dea, _ = _reference(sd, g, nh, steps, dt, dtype=torch.float64)
    model = _edge_model(latent, nh, steps, sd, train_precision, locality)
    g.x.requires_grad_(True)
    g.edge_attr.requires_grad_(True)
    pred = model(g)
    loss = _loss(pred, g, dt)
    loss.backward()
    assert _close(pred["acceleration"], want_out["acceleration"], 1e-5)
    assert _close(pred["temp_rate"], want_out["temp_rate"], 1e-5)
    assert abs(float(loss.detach()) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    ptol = ILL_PTOL if ill else GTOL
    xtol = ILL_XTOL if ill else GTOL
    assert _close(g.x.grad, want_dx, xtol)
    assert g.edge_attr.grad is not None and _close(g.edge_attr.grad, want_dea, xtol)
    got = dict(model.named_parameters())
    for name, ref in sdr.items():
        assert ref.grad is not None and got[name].grad is not None, name
        assert got[name].grad.shape == ref.grad.shape, name
        # one-element gradients (the temperature decoder's output bias): see test_gpu_training.py
        assert _close(got[name].grad, ref.grad, ptol if ref.grad.numel() > 1 or ill else 5 * ptol), name


def test_edge_mode_on_a_general_edge_list():
    """An edge list that is not receiver-sorted (fixed_k == 0: receiver sums through a CSR, no locality order)."""
    n, k, latent, nh, steps = 400, 8, 64, 2, 2
    g, sd, dt = _problem(n, k, latent, nh, steps, seed=77)
    perm = torch.randperm(g.edge_index.shape[1], generator=torch.Generator().manual_seed(3)).to(g.edge_index.device)
    g = Data(x=g.x, edge_index=g.edge_index[:, perm].contiguous(), edge_attr=g.edge_attr[perm].contiguous(), y_acc=g.y_acc,
             y_temp_rate=g.y_temp_rate)
    assert graph_network._graph_arrays(g, n)[2] == 0
    want_loss, sdr, want_dx, want_dea, want_out = _reference(sd, g, nh, steps, dt)
    model = _edge_model(latent, nh, steps, sd)
    g.x.requires_grad_(True)
    g.edge_attr.requires_grad_(True)
    loss = _loss(model(g), g, dt)
    loss.backward()
    assert abs(float(loss.detach()) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    assert _close(g.x.grad, want_dx) and _close(g.edge_attr.grad, want_dea)
    got = dict(model.named_parameters())
    for name, ref in sdr.items():
        assert _close(got[name].grad, ref.grad, GTOL if ref.grad.numel() > 1 else 5 * GTOL), name


def test_edge_attr_gradient_only_when_required():
    """d edge_attr is returned when edge_attr requires it and matches the reference; otherwise none is formed and the
    parameters' gradients are the same bits."""
    g, sd, dt = _problem(500, 16, 32, 2, 2, seed=5)
    want_loss, sdr, want_dx, want_dea, _ = _reference(sd, g, 2, 2, dt)
    runs = []
    for need in (True, False):
        model = _edge_model(32, 2, 2, sd)
        ea = g.edge_attr.detach().clone().requires_grad_(need)
        gg = Data(x=g.x, edge_index=g.edge_index, edge_attr=ea, y_acc=g.y_acc, y_temp_rate=g.y_temp_rate)
        _loss(model(gg), gg, dt).backward()
        runs.append([p.grad.clone() for p in model.parameters()])
        if need:
            assert ea.grad is not None and _close(ea.grad, want_dea)
        else:
            assert ea.grad is None
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))


def test_edge_mode_batch_momentum_and_adam_steps():
    """A batch of three graphs of different sizes with the momentum term: gradients against the oracle; five Adam steps
    lower the loss and move the edge models' weights."""
    graphs, sd, dt = [], None, None
    for s, n in enumerate((300, 417, 250)):
        g, sd0, dt = _problem(n, 8, 32, 2, 2, seed=40 + s)
        graphs.append(g)
        sd = sd or sd0
    batch = Batch.from_data_list(graphs)
    model = _edge_model(32, 2, 2, sd)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    big = Data(x=batch.x, edge_index=batch.edge_index, edge_attr=batch.edge_attr, y_acc=batch.y_acc,
               y_temp_rate=batch.y_temp_rate)
    want_loss, sdr, _, _, _ = _reference(sd, big, 2, 2, dt, batch.batch, 3)

    def step():
        pred = model(batch)
        loss = (torch.nn.functional.mse_loss(pred["acceleration"], batch.y_acc)
                + 0.5 * torch.nn.functional.mse_loss(pred["temp_rate"], batch.y_temp_rate)
                + losses.momentum_conservation_loss(pred["acceleration"], batch, dt, 0.1))
        opt.zero_grad()
        loss.backward()
        return loss.detach()

    l0 = step()
    assert abs(float(l0) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    got = dict(model.named_parameters())
    for name, r in sdr.items():
        assert _close(got[name].grad, r.grad, GTOL if r.grad.numel() > 1 else 5 * GTOL), name
    before = {k: v.detach().clone() for k, v in got.items() if ".edge_model." in k}
    opt.step()
    seen = [float(l0)]
    for _ in range(5):
        seen.append(float(step()))
        opt.step()
    assert seen[-1] < seen[0]
    for k, v in before.items():
        assert not torch.equal(got[k].detach(), v), k


@pytest.mark.parametrize("train_precision", ["fp32", "fp32x3"])
def test_edge_mode_step_is_reproducible(train_precision):
    """A fixed-k graph: two steps give the same gradients bit for bit (every sum over particles or edges in a fixed order)."""
    g, sd, dt = _problem(700, 16, 128, 2, 2, seed=11)
    model = _edge_model(128, 2, 2, sd, train_precision)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        ea = g.edge_attr.detach().clone().requires_grad_(True)
        gg = Data(x=g.x, edge_index=g.edge_index, edge_attr=ea, y_acc=g.y_acc, y_temp_rate=g.y_temp_rate)
        for hint in ("_cgnn_fixed_k", "_cgnn_fixed_k_for", "_cgnn_graph", "_cgnn_order"):
            if hasattr(g, hint):
                setattr(gg, hint, getattr(g, hint))
        _loss(model(gg), gg, dt).backward()
        runs.append([p.grad.clone() for p in model.parameters()] + [ea.grad.clone()])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1], strict=True))


def test_switch_is_inert_in_x_j_mode():
    """message_source="x_j": train_edge_messages = True gives the same outputs and gradients, bit for bit."""
    g, sd, dt = _problem(600, 8, 64, 2, 2, seed=23)
    runs = []
    for switch in (False, True):
        model = graph_network.EncodeProcessDecode(64, 64, 2, 2, 3)
        model.load_state_dict(sd)
        model = model.to(DEV).train()
        model.train_edge_messages = switch
        pred = model(g)
        _loss(pred, g, dt).backward()
        runs.append([pred["acceleration"].detach(), pred["temp_rate"].detach()] +
                    [p.grad.clone() if p.grad is not None else None for p in model.parameters()])
    for a, b in zip(runs[0], runs[1], strict=True):
        assert (a is None and b is None) or torch.equal(a, b)


def test_edge_mode_refusals(monkeypatch):
    """Refused before launch: a (hidden, latent) pair the kernel is not built for; a memory estimate above the free device
    memory (blocks the caching allocator holds reserved but unused count as free); and, without the switch, edge-mode
    training altogether (NotImplementedError naming the switch)."""
    gen = torch.Generator().manual_seed(0)
    sd = _edge_sd(gen, 128, 64, 2)
    lins = [_Lin(sd[f"m.0.{2 * i}.weight"].to(DEV), sd[f"m.0.{2 * i}.bias"].to(DEV)) for i in range(3)]
    lnm = _Lin(sd["m.1.weight"].to(DEV), sd["m.1.bias"].to(DEV))
    with pytest.raises(ops.CgnnError, match="built for"):
        training._TrainEdge(lins, lnm, 128)
    fwd = ops.PackedMLP([(l.weight, l.bias) for l in lins], (lnm.weight, lnm.bias), "fp32", first_layer_cols=(256, 128))
    t = lambda w: w.t().contiguous()  # noqa: E731
    bwd = ops.PackedMLP([(t(lins[0].weight[:, 256:]), None), (t(lins[1].weight), None), (t(lins[2].weight), None)], None,
                        "fp32")
    n, ne = 8, 64
    src = torch.zeros(ne, dtype=torch.int32, device=DEV)
    tab = torch.zeros(n, 64, device=DEV)
    et = ops.TiledRows(ne, 128, DEV)
    with pytest.raises(ops.CgnnError, match="no kernel"):
        ops.edge_mlp_backward(fwd, bwd, tab, tab, src, src, et, torch.zeros(n, 128, device=DEV), None,
                              ops.BackwardScratch(ne, 64, 128, 2, DEV), torch.empty(ne, 128, device=DEV), et.empty_like())
    g, sdm, dt = _problem(300, 8, 32, 2, 2, seed=3)
    model = _edge_model(32, 2, 2, sdm)
    need = training.edge_training_bytes(g.edge_index.shape[1], 32, 32, 2, 2)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need - 1, 1 << 40))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 0)
    with pytest.raises(ops.CgnnError, match="device memory"):
        model(g)
    # blocks the caching allocator holds reserved but unused count as free: the same step runs
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 2)
    pred = model(g)
    assert pred["acceleration"].requires_grad
    monkeypatch.undo()
    model.train_edge_messages = False
    with pytest.raises(NotImplementedError, match="train_edge_messages"):
        model(g)
