"""GPU: gradients of the HIP node-stream backward (cgnn_mlp_backward / cgnn_weight_grad / cgnn_col_dot through
EncodeProcessDecode) against torch autograd on the CPU oracle -- what reference train.py:263 differentiates.

Tolerance: gradients are float32 sums over all particles in a different order than torch's; the bound is
2e-5 of each tensor's largest gradient entry (float32 outputs themselves stay within 1e-5)."""
import pytest
import torch

import backward_checks as bc
from backward_checks import GTOL, Lin as _Lin, close as _close, rand_mlp as _rand_mlp
from cosmology_gnn_simulation_amd import _lib, data_utils, graph_network, losses, ops, synthetic
from cosmology_gnn_simulation_amd.graph import Batch, Data
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("n,fin,fin2,hid,out,nh,ln", [
    (1, 17, 0, 32, 32, 2, True), (1000, 21, 0, 64, 64, 2, True), (333, 17, 0, 128, 128, 1, True),
    (257, 128, 0, 128, 3, 2, False), (64, 64, 0, 64, 1, 3, False), (4100, 128, 128, 128, 128, 2, True),
    (95, 32, 32, 32, 32, 1, True), (700, 64, 64, 64, 64, 3, True),
    (200, 17, 0, 256, 256, 2, True), (300, 256, 256, 256, 256, 2, True), (150, 256, 0, 256, 3, 2, False),    # latent 256 (cfg5)
    # mlp_hidden_size != latent_size (reference config.py:19-20): hidden 128 with latent 64 / 256 -- encoder, round, decoder
    (500, 17, 0, 128, 64, 2, True), (400, 64, 64, 128, 64, 2, True), (300, 64, 0, 128, 3, 2, False),
    (200, 17, 0, 128, 256, 2, True), (300, 256, 256, 128, 256, 1, True), (150, 256, 0, 128, 1, 3, False)])
@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "fp32x3 with the forward recomputed on fp16x2"])
def test_mlp_backward_matches_autograd(n, fin, fin2, hid, out, nh, ln, precision):
    """cgnn_mlp_backward + the parameter-gradient reductions of one MLP against torch autograd on the oracle: exact f32,
    three bf16 terms, and the pairing the processor rounds / decoders train with (recomputed forward on two fp16 terms,
    gradient chain on three bf16 terms).  Besides the 2e-5 of each tensor's largest entry, EVERY row of du1 / du2 is held
    to 2e-5 of its own norm against float64 autograd (backward_checks.py).  For that gate the input rows are
    margin-filtered: a row with a ReLU input at rounding distance from zero (min |a| / max |a| <= 1e-5 over a hidden layer)
    has a discontinuous gradient that any f32 evaluation may get wrong by 1 / sqrt(H), so it is re-drawn from the same
    generator (most seeds have none).  All sizes here run one tile per wave; test_gpu_backward_gates.py runs more."""
    from cosmology_gnn_simulation_amd.training import _TrainMLP
    latent_input = precision.endswith("fp16x2")
    precision = precision.split()[0]
    gen = torch.Generator().manual_seed(n + fin + out)
    sd = _rand_mlp(gen, fin + fin2, hid, out, nh, ln)
    u = torch.randn(n, fin + fin2, generator=gen)
    dy = torch.randn(n, out, generator=gen)
    bc.redraw_fragile_mlp_rows(gen, sd, u, nh, cap=None)
    want64 = bc.mlp_reference(dict(sd=sd, u=u, dy=dy, nh=nh, ln=ln))["du"]
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    u.requires_grad_(True)
    y = cpu_ref.mlp_ln(sd, "m", u, nh) if ln else cpu_ref.mlp(sd, "m.0", u, nh)
    y.backward(dy)

    lins = [_Lin(sd[f"m.0.{2 * i}.weight"].detach().to(DEV), sd[f"m.0.{2 * i}.bias"].detach().to(DEV))
            for i in range(nh + 1)]
    lnm = _Lin(sd["m.1.weight"].detach().to(DEV), sd["m.1.bias"].detach().to(DEV)) if ln else None
    tm = _TrainMLP(lins, lnm, split_at=fin if fin2 else None, precision=precision, latent_input=latent_input)
    assert (tm.rec.precision == _lib.F16X2) == latent_input
    scratch = ops.BackwardScratch(n, hid, max(hid, out, 32), nh, DEV)
    ud = u.detach().to(DEV)
    u1 = ud[:, :fin].contiguous()
    u2 = ud[:, fin:].contiguous() if fin2 else None
    du1, du2, grads = tm.backward(u1, u2, dy.to(DEV), scratch, True, True)
    assert _close(du1, u.grad[:, :fin])
    bc.assert_rows(du1, want64[:, :fin], "du1")
    if fin2:
        assert _close(du2, u.grad[:, fin:])
        bc.assert_rows(du2, want64[:, fin:], "du2")
    names = [f"m.0.{2 * i}.{p}" for i in range(nh + 1) for p in ("weight", "bias")] + (["m.1.weight", "m.1.bias"] if ln else [])
    assert len(grads) == len(names)
    for name, g in zip(names, grads):
        assert g.shape == sd[name].shape
        assert _close(g, sd[name].grad), name


@pytest.mark.parametrize("n,col0,scale", [(1, 0, 1.0), (5000, 128, 1.0), (1025, 0, 1e-7), (70001, 0, 1.0), (33, 64, 1e3)])
def test_weight_grad_three_bf16_terms_is_f32_accurate_and_reproducible(n, col0, scale):
    """cgnn_weight_grad_x3 (128 x 128, precision="fp32x3"): the bf16-matrix-core reduction against float64, no worse than
    the f32-MFMA kernel; tiny gradients (1e-7: far below fp16's range, fine for bf16's) keep their accuracy; the same
    bits on every run (fixed summation order, where the f32 kernel adds row chunks with atomics)."""
    gen = torch.Generator().manual_seed(n + col0)
    g = (torch.randn(n, 128, generator=gen) * scale).to(DEV)
    a = torch.randn(n, 128, generator=gen).to(DEV)
    want = g.double().t() @ a.double()
    want_b = g.double().sum(0)
    outs = []
    for _ in range(2):
        dw = torch.zeros(128, col0 + 128, device=DEV)
        db = torch.zeros(128, device=DEV)
        ops.weight_grad(g, 128, 128, a, 128, n, dw, col0, db, "fp32x3")
        outs.append((dw, db))
    dw, db = outs[0]
    assert torch.equal(dw, outs[1][0]) and torch.equal(db, outs[1][1])
    assert float(dw[:, :col0].abs().sum()) == 0.0
    ref = torch.zeros(128, col0 + 128, device=DEV)
    ops.weight_grad(g, 128, 128, a, 128, n, ref, col0, None)                    # the f32-MFMA kernel
    scale_w = float(want.abs().max())
    err = float((dw[:, col0:].double() - want).abs().max()) / scale_w
    err_ref = float((ref[:, col0:].double() - want).abs().max()) / scale_w
    assert err <= 2e-6 and err <= 4 * err_ref + 2e-7, (err, err_ref)
    assert _close(db, want_b, 1e-5)
    # accumulates into dw like the f32 kernel
    ops.weight_grad(g, 128, 128, a, 128, n, dw, col0, None, "fp32x3")
    assert float((dw[:, col0:].double() - 2 * want).abs().max()) <= 4e-6 * scale_w
    # shapes it does not take (here 128 x 64) run the f32 kernel under the same call
    dw2 = torch.zeros(128, 64, device=DEV)
    a64 = a[:, :64].contiguous()
    ops.weight_grad(g, 128, 128, a64, 64, n, dw2, 0, None, "fp32x3")
    assert _close(dw2, g.double().t() @ a64.double(), 1e-5)


def test_weight_grad_x3_abi_rejects_what_it_cannot_take():
    """The C entry itself (the Python wrapper routes such calls to cgnn_weight_grad before they get here): a leading
    dimension that is not a multiple of 4 -> CGNN_ERR_UNSUPPORTED naming the fallback; a short workspace / NULL pointers
    -> CGNN_ERR_INVALID_ARG; nothing is launched."""
    lib = _lib.load()
    n = 64
    g = torch.randn(n, 130, device=DEV)
    a = torch.randn(n, 128, device=DEV)
    dw = torch.zeros(128, 128, device=DEV)
    ws = torch.empty(lib.cgnn_weight_grad_x3_workspace_bytes(), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.cgnn_weight_grad_x3(g.data_ptr(), 130, a.data_ptr(), 128, n, dw.data_ptr(), 128, 0, None, ws.data_ptr(), ws.numel(), st)
    assert rc == -2 and b"cgnn_weight_grad" in lib.cgnn_last_error()             # CGNN_ERR_UNSUPPORTED
    rc = lib.cgnn_weight_grad_x3(a.data_ptr(), 128, a.data_ptr(), 128, n, dw.data_ptr(), 128, 0, None, ws.data_ptr(), 1024, st)
    assert rc == -1 and b"workspace" in lib.cgnn_last_error()                    # CGNN_ERR_INVALID_ARG
    rc = lib.cgnn_weight_grad_x3(None, 128, a.data_ptr(), 128, n, dw.data_ptr(), 128, 0, None, ws.data_ptr(), ws.numel(), st)
    assert rc == -1
    torch.cuda.synchronize()
    assert float(dw.abs().sum()) == 0.0
    rc = lib.cgnn_col_dot2(a.data_ptr(), 128, None, 128, n, 128, dw.data_ptr(), dw.data_ptr(), st)
    assert rc == -1 and b"cgnn_col_dot2" in lib.cgnn_last_error()


def test_mlp_backward_rejects_unsupported_shapes():
    from cosmology_gnn_simulation_amd.training import _TrainMLP
    gen = torch.Generator().manual_seed(0)
    sd = _rand_mlp(gen, 17, 64, 128, 2, True)             # hidden 64, latent 128: not a pair the kernels are compiled for
    lins = [_Lin(sd[f"m.0.{2 * i}.weight"].to(DEV), sd[f"m.0.{2 * i}.bias"].to(DEV)) for i in range(3)]
    tm = _TrainMLP(lins, _Lin(sd["m.1.weight"].to(DEV), sd["m.1.bias"].to(DEV)))
    scratch = ops.BackwardScratch(8, 64, 128, 2, DEV)
    with pytest.raises(ops.CgnnError, match="no kernel"):
        tm.backward(torch.zeros(8, 17, device=DEV), None, torch.zeros(8, 128, device=DEV), scratch, True)


@pytest.mark.parametrize("n,e,width", [(500, 8000, 128), (300, 4800, 64), (10, 0, 32), (7, 1, 4), (64, 5000, 32)])
def test_csr_build_and_transposed_aggregation(n, e, width):
    gen = torch.Generator().manual_seed(e + n)
    src = torch.randint(0, n, (e,), generator=gen, dtype=torch.int32)
    if e > 1000:
        src[: e // 4] = 3                                   # a hub row long enough for the heap-sort branch
    dst = torch.randint(0, n, (e,), generator=gen, dtype=torch.int32)
    csr = ops.SenderCsr(src.to(DEV), dst.to(DEV), n)
    row_ptr = csr.row_ptr.cpu().long()
    counts = torch.bincount(src.long(), minlength=n)
    assert torch.equal(row_ptr, torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]))      # bit exact
    col = csr.col.cpu()[:e]
    for r in range(n):                                       # each row: that sender's receivers, ascending
        want = torch.sort(dst[src == r]).values
        assert torch.equal(col[row_ptr[r]:row_ptr[r + 1]], want)
    table = torch.randn(n, width, generator=gen)
    got = ops.aggregate_csr(table.to(DEV), csr).cpu()
    want = torch.zeros(n, width, dtype=torch.float64).index_add_(0, src.long(), table[dst.long()].double())
    assert torch.allclose(got.double(), want, rtol=0, atol=1e-5 * max(1.0, float(want.abs().max())))
    again = ops.aggregate_csr(table.to(DEV), ops.SenderCsr(src.to(DEV), dst.to(DEV), n)).cpu()
    assert torch.equal(got, again)                           # fixed summation order: reproducible bit for bit
    # it is the adjoint of the forward aggregation: <A x, y> == <x, A^T y>
    x, y = torch.randn(n, width, generator=gen), torch.randn(n, width, generator=gen)
    ax = ops.aggregate(x.to(DEV), src.to(DEV), dst.to(DEV), n, 0, e).cpu() if e else torch.zeros(n, width)
    aty = ops.aggregate_csr(y.to(DEV), csr).cpu()
    lhs, rhs = float((ax.double() * y.double()).sum()), float((x.double() * aty.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * float((ax.double() * y.double()).abs().sum()) + 1e-6      # float32 rounding only
    # with addends (the residual round's backward, dx + du1 + A^T du2, in one pass): the same bits as the separate adds,
    # also when the output is one of the addends
    a1, a2 = torch.randn(n, width, generator=gen).to(DEV), torch.randn(n, width, generator=gen).to(DEV)
    fused = ops.aggregate_csr(table.to(DEV), csr, add1=a1, add2=a2)
    assert torch.equal(fused, (a1 + a2) + got.to(DEV))
    assert torch.equal(ops.aggregate_csr(table.to(DEV), csr, add2=a2), a2 + got.to(DEV))
    inplace = a1.clone()
    assert ops.aggregate_csr(table.to(DEV), csr, out=inplace, add1=inplace, add2=a2) is inplace
    assert torch.equal(inplace, fused)


def test_csr_build_rejects_out_of_range_keys():
    src = torch.tensor([0, 5, 1], dtype=torch.int32, device=DEV)
    with pytest.raises(ops.CgnnError, match="outside"):
        ops.SenderCsr(src, src, 4)


@pytest.mark.parametrize("n,out,fin,col0", [(1, 3, 128, 0), (5000, 128, 128, 128), (1025, 64, 21, 0), (2047, 32, 64, 0),
                                            (300, 128, 256, 0), (40, 1, 32, 0)])
def test_weight_grad_and_col_dot(n, out, fin, col0):
    gen = torch.Generator().manual_seed(n + out)
    ldg = (out + 31) // 32 * 32
    g = torch.randn(n, ldg, generator=gen)
    a = torch.randn(n, fin, generator=gen)
    dw = torch.zeros(out, col0 + fin, device=DEV)
    db = torch.zeros(out, device=DEV)
    ops.weight_grad(g.to(DEV), ldg, out, a.to(DEV), fin, n, dw, col0, db)
    want = g[:, :out].double().t() @ a.double()
    assert _close(dw[:, col0:], want, 1e-5)
    assert float(dw[:, :col0].abs().sum()) == 0.0
    assert _close(db, g[:, :out].double().sum(0), 1e-5)
    b = torch.randn(n, fin, generator=gen)
    o1, o2 = torch.zeros(fin, device=DEV), torch.zeros(fin, device=DEV)
    ops.col_dot(a.to(DEV), fin, b.to(DEV), fin, n, fin, o1)
    ops.col_dot(a.to(DEV), fin, None, 0, n, fin, o2)
    assert _close(o1, (a.double() * b.double()).sum(0), 1e-5)
    assert _close(o2, a.double().sum(0), 1e-5)
    o3, o4 = torch.zeros(fin, device=DEV), torch.zeros(fin, device=DEV)
    ops.col_dot2(a.to(DEV), fin, b.to(DEV), fin, n, fin, o3, o4)               # both sums from one pass
    assert _close(o3, (a.double() * b.double()).sum(0), 1e-5)
    assert _close(o4, a.double().sum(0), 1e-5)


def _problem(n, k, latent, nh, steps, seed, window=5):
    snap = synthetic.make_snapshot(n, window, seed=seed)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    dt = 0.01
    g = data_utils.preprocess(c[:window].clone(), e[:window].clone(), meta, c[window].clone(), e[window].clone(), 0.0, k,
                              dt, 1.0)
    sd = synthetic.make_state_dict(latent, latent, nh, steps, 3, node_in=g.x.shape[1], edge_in=4, seed=seed + 1)
    return g, sd, dt


def _reference_grads(sd, g, nh, steps, dt, batch=None, num_graphs=1):
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = g.x.cpu().clone().requires_grad_(True)
    out = cpu_ref.encode_process_decode(sdr, x, g.edge_index.cpu().long(), g.edge_attr.cpu(), nh, steps)
    mse = torch.nn.functional.mse_loss
    b = torch.zeros(x.shape[0], dtype=torch.long) if batch is None else batch.cpu().long()
    loss = (mse(out["acceleration"], g.y_acc.cpu()) + 0.5 * mse(out["temp_rate"], g.y_temp_rate.cpu())
            + cpu_ref.momentum_conservation_loss(out["acceleration"], b, num_graphs, dt, 0.1))
    loss.backward()
    return loss.detach(), sdr, x.grad, out


@pytest.mark.parametrize("n,k,latent,nh,steps", [(600, 8, 32, 2, 2), (1500, 16, 128, 2, 3), (900, 8, 64, 1, 4),
                                                  (500, 32, 256, 2, 2)])        # cfg5's latent / k
@pytest.mark.parametrize("locality,train_precision", [(True, "fp32"), (False, "fp32"), (True, "fp32x3")])
def test_training_step_gradients_match_reference_autograd(n, k, latent, nh, steps, locality, train_precision):
    """train_precision "fp32x3": forward and backward GEMMs on three-bf16-term emulated f32 (bf16 matrix cores); same
    gates as the exact-f32 kernels."""
    g, sd, dt = _problem(n, k, latent, nh, steps, seed=n)
    want_loss, sdr, want_dx, want_out = _reference_grads(sd, g, nh, steps, dt)

    model = graph_network.EncodeProcessDecode(latent, latent, nh, steps, 3)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    model.locality_sort = locality
    model.train_precision = train_precision
    g.x.requires_grad_(True)
    pred = model(g)
    assert pred["acceleration"].requires_grad and pred["temp_rate"].requires_grad
    mse = torch.nn.functional.mse_loss
    loss = (mse(pred["acceleration"], g.y_acc) + 0.5 * mse(pred["temp_rate"], g.y_temp_rate)
            + losses.momentum_conservation_loss(pred["acceleration"], g, dt, 0.1))
    loss.backward()
    assert _close(pred["acceleration"], want_out["acceleration"], 1e-5)
    assert _close(pred["temp_rate"], want_out["temp_rate"], 1e-5)
    assert abs(float(loss.detach()) - float(want_loss)) <= 1e-5 * abs(float(want_loss))
    # gradient gate: 2e-5 of each tensor's largest entry (f32 sums over all particles in another order than torch's);
    # 3e-5 at latent 256, where every dot product is twice as long (measured 2.4e-5 on three bf16 terms; exact f32 stays under 2e-5)
    gtol = GTOL if latent <= 128 else 1.5 * GTOL
    assert _close(g.x.grad, want_dx, gtol)
    got = dict(model.named_parameters())
    for name, ref in sdr.items():
        if ".edge_model." in name:
            # the reference's autograd never reaches the edge models: grad stays None on both sides
            assert ref.grad is None and got[name].grad is None, name
        else:
            assert got[name].grad is not None, name
            # a one-element gradient (the temperature decoder's output bias) is a single f32 sum over all particles of
            # terms that cancel: sum |terms| / |sum| = 432 in the [900-8-64-1-4] case, so "relative to its largest
            # entry" means relative to that small result.  The HIP value has the same bits on every run (8.7e-6 from
            # the float64 sum); the torch CPU reference moves with the box's thread count (3.2e-5 apart was seen once
            # in a dozen runs).  scripts/dev/check_scalar_grad.py prints these numbers.
            assert _close(got[name].grad, ref.grad, gtol if ref.grad.numel() > 1 else 5 * gtol), name


@pytest.mark.parametrize("window,latent", [(10, 128), (16, 64)])
@pytest.mark.parametrize("train_precision", ["fp32", "fp32x3"])
def test_training_step_with_a_window_longer_than_eight_frames(window, latent, train_precision):
    """--window_size > 8 (reference config.py:18; data_utils.py:138-145 builds 3 (W - 1) + W node features: 37 at W = 10, 61 at
    W = 16): the encoder's backward takes up to 64 input features (two 32-feature tiles, the second one ragged).  Same
    gates as the W = 5 models."""
    n, k, nh, steps = 800, 8, 2, 2
    g, sd, dt = _problem(n, k, latent, nh, steps, seed=300 + window, window=window)
    assert g.x.shape[1] == 3 * (window - 1) + window
    want_loss, sdr, want_dx, want_out = _reference_grads(sd, g, nh, steps, dt)
    model = graph_network.EncodeProcessDecode(latent, latent, nh, steps, 3)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    model.train_precision = train_precision
    g.x.requires_grad_(True)
    pred = model(g)
    mse = torch.nn.functional.mse_loss
    loss = (mse(pred["acceleration"], g.y_acc) + 0.5 * mse(pred["temp_rate"], g.y_temp_rate)
            + losses.momentum_conservation_loss(pred["acceleration"], g, dt, 0.1))
    loss.backward()
    assert _close(pred["acceleration"], want_out["acceleration"], 1e-5)
    assert _close(pred["temp_rate"], want_out["temp_rate"], 1e-5)
    assert _close(g.x.grad, want_dx, GTOL)
    got = dict(model.named_parameters())
    for name, ref in sdr.items():
        if ".edge_model." in name:
            assert ref.grad is None and got[name].grad is None, name
        else:
            assert got[name].grad is not None, name
            assert _close(got[name].grad, ref.grad, GTOL if ref.grad.numel() > 1 else 5 * GTOL), name
    # the same window through the inference kernels (every node precision the bench presets use)
    model.eval()
    for node_precision in ("fp32", "fp16x2"):
        model.node_precision = node_precision
        with torch.no_grad():
            out = model(g)
        assert _close(out["acceleration"], want_out["acceleration"], 1e-5), node_precision
        assert _close(out["temp_rate"], want_out["temp_rate"], 1e-5), node_precision
    # 65 features and more: refused (the backward is compiled for two input tiles)
    g17, sd17, _ = _problem(300, 8, 64, 2, 1, seed=9, window=17)
    m17 = graph_network.EncodeProcessDecode(64, 64, 2, 1, 3)
    m17.load_state_dict(sd17)
    m17 = m17.to(DEV).train()
    with pytest.raises(ops.CgnnError, match="64 node input features"):
        m17(g17)


@pytest.mark.parametrize("n,k,latent,hidden,nh,steps", [(700, 8, 64, 128, 2, 3), (400, 16, 256, 128, 2, 2)])
@pytest.mark.parametrize("train_precision", ["fp32", "fp32x3"])
def test_training_step_with_hidden_size_other_than_latent(n, k, latent, hidden, nh, steps, train_precision):
    """The reference passes latent_size and mlp_hidden_size independently (config.py:19-20, train.py:165-171): a training
    step with hidden 128 and latent 64 / 256 against torch autograd on the oracle, same gates as the square models."""
    window, seed = 5, n
    snap = synthetic.make_snapshot(n, window, seed=seed)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    dt = 0.01
    g = data_utils.preprocess(c[:window].clone(), e[:window].clone(), meta, c[window].clone(), e[window].clone(), 0.0, k,
                              dt, 1.0)
    sd = synthetic.make_state_dict(latent, hidden, nh, steps, 3, node_in=g.x.shape[1], edge_in=4, seed=seed + 1)
    want_loss, sdr, want_dx, want_out = _reference_grads(sd, g, nh, steps, dt)
    model = graph_network.EncodeProcessDecode(latent, hidden, nh, steps, 3)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    model.train_precision = train_precision
    g.x.requires_grad_(True)
    pred = model(g)
    mse = torch.nn.functional.mse_loss
    loss = (mse(pred["acceleration"], g.y_acc) + 0.5 * mse(pred["temp_rate"], g.y_temp_rate)
            + losses.momentum_conservation_loss(pred["acceleration"], g, dt, 0.1))
    loss.backward()
    assert _close(pred["acceleration"], want_out["acceleration"], 1e-5)
    assert _close(pred["temp_rate"], want_out["temp_rate"], 1e-5)
    gtol = GTOL if latent <= 128 else 1.5 * GTOL
    assert _close(g.x.grad, want_dx, gtol)
    got = dict(model.named_parameters())
    for name, ref in sdr.items():
        if ".edge_model." in name:
            assert ref.grad is None and got[name].grad is None, name
        else:
            assert got[name].grad is not None and got[name].grad.shape == ref.grad.shape, name
            assert _close(got[name].grad, ref.grad, gtol if ref.grad.numel() > 1 else 5 * gtol), name


def test_training_on_a_batch_of_graphs_and_optimizer_step():
    """train.py:233-264 shape: several graphs batched, Adam step, second forward sees the updated weights."""
    graphs, sd, dt = [], None, None
    for s in range(2):
        g, sd0, dt = _problem(400, 8, 32, 2, 2, seed=10 + s)
        graphs.append(g)
        sd = sd or sd0
    batch = Batch.from_data_list(graphs)
    model = graph_network.EncodeProcessDecode(32, 32, 2, 2, 3)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    opt = torch.optim.Adam([p for n, p in model.named_parameters()], lr=1e-3)
    mse = torch.nn.functional.mse_loss

    def step():
        pred = model(batch)
        loss = (mse(pred["acceleration"], batch.y_acc) + mse(pred["temp_rate"], batch.y_temp_rate)
                + losses.momentum_conservation_loss(pred["acceleration"], batch, dt, 0.1))
        opt.zero_grad()
        loss.backward()
        return loss.detach()

    l0 = step()
    # same batch on the oracle
    big = Data(x=batch.x, edge_index=batch.edge_index, edge_attr=batch.edge_attr, y_acc=batch.y_acc,
               y_temp_rate=batch.y_temp_rate)
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = cpu_ref.encode_process_decode(sdr, big.x.cpu(), big.edge_index.cpu().long(), big.edge_attr.cpu(), 2, 2)
    ref = (mse(out["acceleration"], big.y_acc.cpu()) + mse(out["temp_rate"], big.y_temp_rate.cpu())
           + cpu_ref.momentum_conservation_loss(out["acceleration"], batch.batch.cpu().long(), 2, dt, 0.1))
    ref.backward()
    assert abs(float(l0) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    got = dict(model.named_parameters())
    for name, r in sdr.items():
        if ".edge_model." not in name:
            assert _close(got[name].grad, r.grad), name
    opt.step()
    losses_seen = [float(l0)]
    for _ in range(5):
        losses_seen.append(float(step()))
        opt.step()
    assert losses_seen[-1] < losses_seen[0]          # the packed weights follow the optimizer


def test_training_rejects_edge_message_source():
    g, sd, dt = _problem(300, 8, 32, 2, 1, seed=3)
    model = graph_network.EncodeProcessDecode(32, 32, 2, 1, 3)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    model.message_source = "edge"
    with pytest.raises(NotImplementedError):
        model(g)
    with torch.no_grad():
        model(g)                                       # inference in that mode still works


def test_training_with_the_edge_stream_switched_on_changes_no_output_and_no_gradient():
    """model.train_edge_stream runs the edge stream's forward inside the training step (the reference computes it although
    nothing reads it; the default skips it and every step time quoted says so): outputs and gradients keep
    their bits, and the stream it runs is the inference one."""
    g, sd, dt = _problem(700, 16, 128, 2, 3, seed=21)
    outs = []
    for on in (False, True):
        model = graph_network.EncodeProcessDecode(128, 128, 2, 3, 3)
        model.load_state_dict(sd)
        model = model.to(DEV).train()
        model.edge_precision, model.node_precision = "bf16", "fp16x2"
        model.train_edge_stream = on
        pred = model(g)
        (pred["acceleration"].square().mean() + pred["temp_rate"].square().mean()).backward()
        outs.append((pred["acceleration"].detach().clone(), pred["temp_rate"].detach().clone(),
                     {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2].keys() == outs[1][2].keys()
    for k in outs[0][2]:
        assert torch.equal(outs[0][2][k], outs[1][2][k]), k
    # what it ran: the edge stream of the inference forward on the training forward's node latents (f32 node path there,
    # fp16x2 here: the bf16 edge operands hide the difference)
    from cosmology_gnn_simulation_amd import training
    model.eval()
    with torch.no_grad():
        ref = model.forward_with_latents(g)["edge_latent"]
    assert bool(torch.isfinite(ref).all())


@pytest.mark.parametrize("n,width", [(70_001, 128), (300_000, 256), (513, 3), (1, 64)])
def test_column_sums_have_the_same_bits_on_every_run(n, width):
    """LayerNorm's dgamma / dbeta and the bias gradients are column sums over all particles: cgnn_col_dot_ordered adds the
    per-workgroup partial sums in a fixed order (the atomic forms cgnn_col_dot / cgnn_col_dot2 do not), so a training
    step's affine and bias gradients are reproducible.  Also its error behaviour at the C ABI."""
    gen = torch.Generator().manual_seed(n + width)
    a = torch.randn(n, width, generator=gen).to(DEV)
    b = torch.randn(n, width, generator=gen).to(DEV)
    runs = []
    for _ in range(4):
        o_ab, o_a = torch.zeros(width, device=DEV), torch.zeros(width, device=DEV)
        ops.col_dot2(a, width, b, width, n, width, o_ab, o_a)
        o_s = torch.zeros(width, device=DEV)
        ops.col_dot(a, width, None, 0, n, width, o_s)
        runs.append((o_ab.clone(), o_a.clone(), o_s.clone()))
        # (other work in between: the order must not depend on what ran before)
        torch.randn(1 << 20, device=DEV).sum()
    for r in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(r, runs[0]))
    assert torch.equal(runs[0][1], runs[0][2])                                  # the same column sums through either entry
    assert _close(runs[0][0], (a.double() * b.double()).sum(0).float(), 1e-5)
    assert _close(runs[0][1], a.double().sum(0).float(), 1e-5)
    # outputs are accumulated into, like the atomic forms
    o = torch.ones(width, device=DEV)
    ops.col_dot(a, width, None, 0, n, width, o)
    assert _close(o - 1, a.double().sum(0).float(), 1e-4)
    lib = _lib.load()
    ws = torch.empty(16, dtype=torch.uint8, device=DEV)                         # too small
    rc = lib.cgnn_col_dot_ordered(a.data_ptr(), width, None, 0, n, width, o.data_ptr(), None, ws.data_ptr(), ws.numel(), None)
    assert (rc != 0) == (lib.cgnn_col_dot_workspace_bytes(n, width) > 16)
    rc = lib.cgnn_col_dot_ordered(a.data_ptr(), width, None, 0, n, width, o.data_ptr(), o.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == -1 and b"cgnn_col_dot_ordered" in lib.cgnn_last_error()      # out_a without b


@pytest.mark.parametrize("n,out,fin,col0", [(70_001, 128, 17, 0), (300_000, 3, 128, 0), (2049, 1, 128, 0), (50_000, 64, 64, 64),
                                            (40_000, 256, 256, 0), (9, 128, 21, 3)])
def test_weight_gradients_of_every_shape_have_the_same_bits_on_every_run(n, out, fin, col0):
    """cgnn_weight_grad_ordered (what ops.weight_grad runs for everything but the 128 x 128 Linears, which have
    cgnn_weight_grad_x3): partial products per row chunk, added in a fixed order -- with the column sums above and the x3
    kernel a whole training step's gradients are reproducible."""
    gen = torch.Generator().manual_seed(n + out + fin)
    ldg = (out + 31) // 32 * 32
    g = torch.randn(n, ldg, generator=gen).to(DEV)
    a = torch.randn(n, fin, generator=gen).to(DEV)
    runs = []
    for _ in range(3):
        dw = torch.zeros(out, col0 + fin, device=DEV)
        db = torch.zeros(out, device=DEV)
        ops.weight_grad(g, ldg, out, a, fin, n, dw, col0, db, "fp32")
        runs.append((dw.clone(), db.clone()))
        torch.randn(1 << 20, device=DEV).sum()
    for dw, db in runs[1:]:
        assert torch.equal(dw, runs[0][0]) and torch.equal(db, runs[0][1])
    want = g[:, :out].double().t() @ a.double()
    assert _close(runs[0][0][:, col0:], want.float(), 1e-5)
    assert float(runs[0][0][:, :col0].abs().sum()) == 0.0
    assert _close(runs[0][1], g[:, :out].double().sum(0).float(), 1e-5)


def test_a_training_step_is_reproducible_bit_for_bit():
    g, sd, dt = _problem(3000, 16, 128, 2, 3, seed=77)
    grads = []
    for _ in range(2):
        model = graph_network.EncodeProcessDecode(128, 128, 2, 3, 3)
        model.load_state_dict(sd)
        model = model.to(DEV).train()
        model.train_precision = "fp32x3"
        pred = model(g)
        mse = torch.nn.functional.mse_loss
        (mse(pred["acceleration"], g.y_acc) + 0.5 * mse(pred["temp_rate"], g.y_temp_rate)).backward()
        grads.append({k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
