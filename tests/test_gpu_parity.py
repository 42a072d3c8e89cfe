"""GPU: the HIP path (through the C ABI) against the CPU oracle and the committed golden fixtures.

Tolerances: integer / index work bit-exact; fp32 kernels <= 1e-5 relative on outputs;
bf16 edge stream has its own stated bound (3e-2 relative L2)."""
import numpy as np
import pytest
import torch

from conftest import edge_index_from, rel_err, rel_l2
from cosmology_gnn_simulation_amd import data_utils, graph_network, losses, one_step, ops, synthetic
from cosmology_gnn_simulation_amd.graph import Batch, Data
from gather_checks import _kernel_order_sum
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
W = 5
TOL = 1e-5


def _model(g, **knobs):
    m = graph_network.EncodeProcessDecode(int(g["latent"]), int(g["latent"]), int(g["nh"]), int(g["steps"]), 3)
    m.load_state_dict(g["state_dict"])
    m = m.to(DEV).eval()
    for k, v in knobs.items():
        setattr(m, k, v)
    return m


def _graph(g):
    return Data(x=torch.from_numpy(g["x"]).to(DEV), edge_index=edge_index_from(g).to(DEV),
                edge_attr=torch.from_numpy(g["edge_attr"]).to(DEV))


# ------------------------------------------------------------------ unit kernels
@pytest.mark.parametrize("n,fin,hid,out,nh,ln", [(1, 17, 32, 32, 2, True), (1000, 4, 64, 64, 2, True),
                                                  (333, 17, 128, 128, 1, True), (257, 128, 128, 3, 2, False),
                                                  (64, 64, 64, 1, 3, False), (100, 17, 128, 64, 2, True),
                                                  (40, 9, 256, 256, 2, True)])
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-6), ("fp32x3", 2e-6), ("fp16x2", 2e-6), ("bf16", 3e-2)])
def test_mlp_rows(n, fin, hid, out, nh, ln, prec, tol):
    gen = torch.Generator().manual_seed(n + fin)
    lin, sd, dims = [], {}, [fin] + [hid] * nh + [out]
    for i in range(nh + 1):
        w = (torch.rand(dims[i + 1], dims[i], generator=gen) * 2 - 1) / dims[i] ** 0.5
        b = torch.rand(dims[i + 1], generator=gen) - 0.5
        lin.append((w.to(DEV), b.to(DEV)))
        sd[f"m.0.{2 * i}.weight"], sd[f"m.0.{2 * i}.bias"] = w, b
    lnp = None
    if ln:
        sd["m.1.weight"], sd["m.1.bias"] = 1 + 0.1 * torch.randn(out, generator=gen), 0.1 * torch.randn(out, generator=gen)
        lnp = (sd["m.1.weight"].to(DEV), sd["m.1.bias"].to(DEV))
    x = torch.randn(n, fin, generator=gen)
    want = cpu_ref.mlp_ln(sd, "m", x, nh) if ln else cpu_ref.mlp(sd, "m.0", x, nh)
    got = ops.mlp_rows(ops.PackedMLP(lin, lnp, prec), x.to(DEV)).cpu()
    assert got.shape == want.shape
    assert rel_l2(got, want) <= tol


@pytest.mark.parametrize("n,k,width", [(1000, 16, 128), (77, 8, 64), (5, 32, 256), (300, 3, 32)])
def test_aggregate_fixed_k_is_exact_segment_sum(n, k, width):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, width, generator=gen)
    src = torch.randint(0, n, (n * k,), generator=gen)
    dst = torch.arange(n).repeat_interleave(k)
    got = ops.aggregate(x.to(DEV), src.to(DEV), None, n, fixed_k=k).cpu()
    assert torch.equal(got, _kernel_order_sum(x[src].view(n, k, width)))   # same summation order: bit exact
    ref = cpu_ref.propagate_add(x, torch.stack([src, dst]))
    assert rel_err(got, ref) <= 1e-6


@pytest.mark.parametrize("n,e,width,sorted_dst", [(500, 8000, 128, True), (500, 8000, 64, False), (10, 0, 32, True),
                                                  (7, 1, 32, False), (2000, 50001, 256, False), (3, 1000, 32, False),
                                                  (40000, 333333, 128, True), (999, 31, 128, False), (64, 5000, 36, False),
                                                  (5000, 80000, 64, True)])
def test_aggregate_general_edge_list(n, e, width, sorted_dst):
    """General scatter-add (fixed_k = 0): widths 32 / 64 / 128 / 256 take the contiguous-atomic kernel (run-length
    reduction + LDS-transposed 256-byte atomic instructions), other widths the scalar-atomic one; destinations with
    thousands of contributions (n = 3), partial last groups, empty lists."""
    gen = torch.Generator().manual_seed(e + 1)
    x = torch.randn(n, width, generator=gen)
    src = torch.randint(0, n, (e,), generator=gen)
    dst = torch.randint(0, n, (e,), generator=gen)
    if sorted_dst:
        dst = dst.sort().values
    got = ops.aggregate(x.to(DEV), src.to(DEV), dst.to(DEV), n, fixed_k=0, num_edges=e).cpu()
    want = cpu_ref.propagate_add(x, torch.stack([src, dst])) if e else torch.zeros(n, width)
    assert torch.allclose(got, want, rtol=0, atol=1e-5 * max(1.0, float(want.abs().max())))
    # messages indexed by edge (message_source="edge")
    msg = torch.randn(e, width, generator=gen)
    got2 = ops.aggregate(msg.to(DEV), None, dst.to(DEV), n, fixed_k=0, num_edges=e).cpu() if e else torch.zeros(n, width)
    want2 = torch.zeros(n, width).index_add_(0, dst, msg)
    assert torch.allclose(got2, want2, rtol=0, atol=1e-5 * max(1.0, float(want2.abs().max())))


@pytest.mark.parametrize("n,k,box,seed", [(256, 8, 1.0, 1), (1000, 16, 1.0, 2), (3000, 16, 25.0, 3), (40, 32, 1.0, 4),
                                          (5, 8, 1.0, 5), (20000, 16, 1.0, 6), (2048, 33, 1.0, 7)])
def test_knn_periodic_bit_exact(n, k, box, seed):
    gen = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=gen) * box
    ei, ea = cpu_ref.knn_periodic(pos, box, k)
    snd, attr, order = ops.knn_periodic(pos.to(DEV), box, k, want_order=True)
    assert torch.equal(snd.cpu().long(), ei[0])                     # indices: bit exact, same order
    assert torch.allclose(attr.cpu(), ea, rtol=0, atol=1e-6 * box)
    assert torch.equal(attr.cpu()[:, :3], ea[:, :3])               # displacements are single subtractions
    assert sorted(order.cpu().tolist()) == list(range(n))          # the locality order is a permutation


def test_knn_clustered_positions_bit_exact():
    """Strongly non-uniform input (tight clumps on a sparse background, the regime of real cosmological
    snapshots): crowded and empty cells, neighbours many shells away, clumps straddling the periodic boundary."""
    gen = torch.Generator().manual_seed(17)
    centers = torch.rand(12, 3, generator=gen)
    centers[0] = torch.tensor([0.999, 0.001, 0.5])                  # a clump on the box corner/edge
    clumps = (centers.repeat_interleave(250, 0) + 0.004 * torch.randn(3000, 3, generator=gen)) % 1.0
    pos = torch.cat([clumps, torch.rand(500, 3, generator=gen)]).float()
    for k in (8, 16):
        ei, ea = cpu_ref.knn_periodic(pos, 1.0, k)
        snd, attr, _ = ops.knn_periodic(pos.to(DEV), 1.0, k)
        assert torch.equal(snd.cpu().long(), ei[0])
        assert torch.equal(attr.cpu()[:, :3], ea[:, :3])


def test_knn_query_subset_and_duplicates():
    gen = torch.Generator().manual_seed(9)
    pos = torch.rand(500, 3, generator=gen)
    pos[10] = pos[3]                                               # coincident particles: tie broken by index
    ei, _ = cpu_ref.knn_periodic(pos, 1.0, 8)
    q = torch.tensor([3, 10, 499, 0], dtype=torch.int32)
    snd, _, _ = ops.knn_periodic(pos.to(DEV), 1.0, 8, query_ids=q.to(DEV))
    want = ei[0].view(500, 8)[q.long()].reshape(-1)
    assert torch.equal(snd.cpu().long(), want)
    assert want.view(4, 8)[1, 0].item() == 3                       # query 10's nearest is particle 3 (lower index)


def test_segment_colsum_and_momentum(golden_tiny):
    g = golden_tiny
    acc = torch.from_numpy(g["acceleration"])
    b = Data(num_graphs=1, batch=None)
    got = float(losses.momentum_conservation_loss(acc.to(DEV), b, g["metadata"]["dt"], 1.0))
    assert abs(got - float(g["momentum"])) <= 1e-6 * abs(float(g["momentum"]))
    # several graphs, ragged sizes
    gen = torch.Generator().manual_seed(0)
    a = torch.randn(7000, 3, generator=gen)
    batch = torch.cat([torch.full((m,), i) for i, m in enumerate([1, 2999, 0, 4000])]).long()
    want = cpu_ref.momentum_conservation_loss(a, batch, 4, 0.01, 0.5)
    got = losses.momentum_conservation_loss(a.to(DEV), Data(num_graphs=4, batch=batch.to(DEV)), 0.01, 0.5)
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want))


def test_gather_scatter_rows():
    gen = torch.Generator().manual_seed(0)
    t = torch.randn(100, 128, generator=gen)
    idx = torch.randperm(100, generator=gen)[:37].int()
    got = ops.gather_rows(t.to(DEV), idx.to(DEV)).cpu()
    assert torch.equal(got, t[idx.long()])
    back = torch.zeros(100, 128, device=DEV)
    ops.scatter_rows(got.to(DEV), idx.to(DEV), back)
    assert torch.equal(back.cpu()[idx.long()], t[idx.long()])
    t3 = torch.randn(50, 3, generator=gen)
    assert torch.equal(ops.gather_rows(t3.to(DEV), idx[:9].to(DEV) % 50).cpu(), t3[(idx[:9] % 50).long()])


@pytest.mark.parametrize("n,width", [(1, 32), (1000, 64), (4097, 128), (33, 256)])
def test_tiled_layout_roundtrip(n, width):
    x = torch.randn(n, width, generator=torch.Generator().manual_seed(n))
    t = ops.TiledRows.from_rows(x.to(DEV))
    assert t.buf.shape[0] == ((n + 31) // 32) * 32
    assert torch.equal(t.to_rows().cpu(), x)                       # pure data movement: bit exact
    # the documented address map (include/cgnn.h): element (row, f) of tile T
    row, f = n - 1, width - 3
    T, r = divmod(row, 32)
    tt, rem = divmod(f, 32)
    g, rem = divmod(rem, 8)
    h, c = divmod(rem, 4)
    off = T * 32 * width + ((4 * tt + g) * 64 + 32 * h + r) * 4 + c
    assert t.buf.view(-1)[off].item() == x[row, f].item()


@pytest.mark.parametrize("n,k,width", [(77, 13, 32), (500, 16, 128), (64, 8, 64), (9, 32, 256)])
def test_aggregate_tiled_messages(n, k, width):
    gen = torch.Generator().manual_seed(k)
    msg = torch.randn(n * k, width, generator=gen)
    dst = torch.arange(n).repeat_interleave(k)
    t = ops.TiledRows.from_rows(msg.to(DEV))
    want = _kernel_order_sum(msg.view(n, k, width))
    assert torch.equal(ops.aggregate(t, None, None, n, fixed_k=k).cpu(), want)
    got = ops.aggregate(t, None, dst.to(DEV), n, fixed_k=0).cpu()          # general path on the tiled table
    assert torch.allclose(got, want, rtol=0, atol=1e-5 * float(want.abs().max()))


# (3e-2 is the stated bf16 bound against the f32 oracle; the per-row / per-element gates of the bf16 kernels against an
# emulation of their own arithmetic live in test_gpu_bf16_kernels.py)
@pytest.mark.parametrize("fmt,tol", [("fp32", 2e-6), ("bf16", 3e-2), ("bf16_n16", 3e-2)])
@pytest.mark.parametrize("n,k,d", [(300, 8, 32), (1000, 16, 128), (70, 5, 64), (1000, 32, 256), (77, 7, 256)])
def test_edge_block_kernel_variants(fmt, tol, n, k, d):
    """Every edge-kernel variant (exact f32, 32-row bf16, 16-row bf16) against the oracle's edge update."""
    gen = torch.Generator().manual_seed(n + d)
    E = n * k
    x = torch.randn(n, d, generator=gen)
    e = torch.randn(E, d, generator=gen)
    src = torch.randint(0, n, (E,), generator=gen)
    dst = torch.arange(n).repeat_interleave(k)
    sd = {"m.0.0.weight": (torch.rand(d, 3 * d, generator=gen) * 2 - 1) / (3 * d) ** 0.5, "m.0.0.bias": torch.rand(d, generator=gen) - 0.5,
          "m.0.2.weight": (torch.rand(d, d, generator=gen) * 2 - 1) / d ** 0.5, "m.0.2.bias": torch.rand(d, generator=gen) - 0.5,
          "m.0.4.weight": (torch.rand(d, d, generator=gen) * 2 - 1) / d ** 0.5, "m.0.4.bias": torch.rand(d, generator=gen) - 0.5,
          "m.1.weight": 1 + 0.1 * torch.randn(d, generator=gen), "m.1.bias": 0.1 * torch.randn(d, generator=gen)}
    want = e + cpu_ref.mlp_ln(sd, "m", torch.cat([x[src], x[dst], e], dim=-1), 2)
    dev = lambda t: t.to(DEV)  # noqa: E731
    w1, b1 = dev(sd["m.0.0.weight"]), dev(sd["m.0.0.bias"])
    lin = [(w1, b1), (dev(sd["m.0.2.weight"]), dev(sd["m.0.2.bias"])), (dev(sd["m.0.4.weight"]), dev(sd["m.0.4.bias"]))]
    mlp = ops.PackedMLP(lin, (dev(sd["m.1.weight"]), dev(sd["m.1.bias"])), fmt, first_layer_cols=(2 * d, d))
    wprec = "fp32" if fmt == "fp32" else "bf16"
    ws, wd = ops.PackedLinear(w1, None, wprec, 0, d), ops.PackedLinear(w1, b1, wprec, d, d)
    ps, pd = ops.project_nodes(ws, wd, dev(x), None, None, ops.p_table_format(mlp.precision))
    et = ops.TiledRows.from_rows(dev(e))
    upd = et.empty_like()
    got = ops.edge_block(mlp, ps, pd, dev(src), dev(dst), et, None, upd, True)
    assert rel_l2(got.to_rows().cpu(), want) <= tol
    assert rel_l2((got.to_rows() - upd.to_rows()).cpu(), e) <= 1e-6      # e_out - e_upd == e_in (f32 residual)


@pytest.mark.parametrize("n,k,d,mode", [(500, 16, 128, "x_j"), (333, 8, 64, "x_j"), (500, 16, 64, "edge"), (77, 8, 32, "edge")])
def test_fused_aggregation_in_edge_kernel_is_bit_identical(n, k, d, mode):
    """cgnn_edge_block's fused aggregate (cross-lane reduction) == the stand-alone cgnn_aggregate, bit for bit."""
    gen = torch.Generator().manual_seed(n + k)
    E = n * k
    x = torch.randn(n, d, generator=gen).to(DEV)
    e = ops.TiledRows.from_rows(torch.randn(E, d, generator=gen).to(DEV))
    src = torch.randint(0, n, (E,), generator=gen).int().to(DEV)
    dst = torch.arange(n).repeat_interleave(k).int().to(DEV)
    w = lambda o, i: ((torch.rand(o, i, generator=gen) * 2 - 1) / i ** 0.5).to(DEV)  # noqa: E731
    b = lambda o: (torch.rand(o, generator=gen) - 0.5).to(DEV)                        # noqa: E731
    w1, b1 = w(d, 3 * d), b(d)
    mlp = ops.PackedMLP([(w1, b1), (w(d, d), b(d)), (w(d, d), b(d))], (1 + 0.1 * b(d), 0.1 * b(d)), "bf16_n16",
                        first_layer_cols=(2 * d, d))
    ws, wd = ops.PackedLinear(w1, None, "bf16", 0, d), ops.PackedLinear(w1, b1, "bf16", d, d)
    ps, pd = ops.project_nodes(ws, wd, x, None, None, ops.p_table_format(mlp.precision))
    upd = e.empty_like()
    out_a = ops.edge_block(mlp, ps, pd, src, dst, e, None, upd, True)
    want = ops.aggregate(x, src, dst, n, k) if mode == "x_j" else ops.aggregate(upd, None, dst, n, k)
    agg = torch.full((n, d), float("nan"), device=DEV)
    out_b = ops.edge_block(mlp, ps, pd, src, dst, e, None, None, True, agg_out=agg,
                           x_gather=x if mode == "x_j" else None, seg_k=k)
    assert torch.equal(out_a.to_rows(), out_b.to_rows())
    assert torch.equal(agg, want)


# ------------------------------------------------------------------ blocks and model vs golden
@pytest.mark.parametrize("prec,tol_x,tol_e", [("fp32", TOL, TOL), ("bf16", 3e-2, 3e-2)])
def test_interaction_block_vs_reference_fixture(golden_tiny, prec, tol_x, tol_e):
    g = golden_tiny
    m = _model(g, node_precision=prec, edge_precision=prec)
    net = m.processor[0]
    net.node_precision = net.edge_precision = prec
    d = Data(x=torch.from_numpy(g["enc_x"]).to(DEV), edge_index=edge_index_from(g).to(DEV),
             edge_attr=torch.from_numpy(g["enc_edge"]).to(DEV))
    with torch.no_grad():
        out = net(d)
    assert rel_l2(out.x.cpu(), torch.from_numpy(g["block0_x"])) <= tol_x
    assert rel_l2(out.edge_attr.cpu(), torch.from_numpy(g["block0_edge"])) <= tol_e
    if prec == "fp32":
        assert rel_err(out.x.cpu(), torch.from_numpy(g["block0_x"])) <= TOL
        assert rel_err(out.edge_attr.cpu(), torch.from_numpy(g["block0_edge"])) <= TOL


def test_encoder_vs_reference_fixture(golden_tiny):
    g = golden_tiny
    m = _model(g)
    with torch.no_grad():
        out = m.encoder(_graph(g))
    assert rel_err(out.x.cpu(), torch.from_numpy(g["enc_x"])) <= TOL
    assert rel_err(out.edge_attr.cpu(), torch.from_numpy(g["enc_edge"])) <= TOL


def test_model_fp32_vs_reference_fixture(golden):
    g = golden
    with torch.no_grad():
        out = _model(g)(_graph(g))
    assert set(out) == {"acceleration", "temp_rate"}
    assert rel_err(out["acceleration"].cpu(), torch.from_numpy(g["acceleration"])) <= TOL
    assert rel_err(out["temp_rate"].cpu(), torch.from_numpy(g["temp_rate"])) <= TOL


@pytest.mark.parametrize("node_precision", ["fp32x3", "fp16x2"])
def test_model_emulated_f32_node_path_meets_fp32_gate(golden, node_precision):
    """node_precision="fp32x3": f32 emulated by three bf16 terms on the bf16 matrix cores (6 MFMAs per product
    block); "fp16x2": by two fp16 terms (3 MFMAs).  Both must hold the same 1e-5 gate as the exact-f32 kernels,
    against the reference fixtures."""
    g = golden
    with torch.no_grad():
        out = _model(g, node_precision=node_precision, edge_precision="bf16")(_graph(g))
    assert rel_err(out["acceleration"].cpu(), torch.from_numpy(g["acceleration"])) <= TOL
    assert rel_err(out["temp_rate"].cpu(), torch.from_numpy(g["temp_rate"])) <= TOL


def test_model_bf16_edge_stream_keeps_fp32_outputs(golden):
    """cfg3 precision: bf16 edge MLP / fp32 node path.  In reference-faithful mode the outputs do not depend on
    the edge stream, so they still meet the fp32 gate; the edge latents carry the bf16 bound."""
    g = golden
    with torch.no_grad():
        out = _model(g, edge_precision="bf16").forward_with_latents(_graph(g))
        ref = cpu_ref.encode_process_decode(g["state_dict"], torch.from_numpy(g["x"]), edge_index_from(g),
                                            torch.from_numpy(g["edge_attr"]), int(g["nh"]), int(g["steps"]),
                                            return_latents=True)
    assert rel_err(out["acceleration"].cpu(), torch.from_numpy(g["acceleration"])) <= TOL
    assert rel_err(out["temp_rate"].cpu(), torch.from_numpy(g["temp_rate"])) <= TOL
    assert rel_l2(out["edge_latent"].cpu(), ref["edge_latent"]) <= 3e-2
    assert rel_err(out["x_latent"].cpu(), ref["x_latent"]) <= TOL


def test_model_edge_message_mode(golden):
    """message_source='edge' (not reference behaviour): against the restatement-only vectors."""
    g = golden
    with torch.no_grad():
        out = _model(g, message_source="edge")(_graph(g))
    assert rel_err(out["acceleration"].cpu(), torch.from_numpy(g["edge_mode_acceleration_cpuref"])) <= 2e-5
    assert rel_err(out["temp_rate"].cpu(), torch.from_numpy(g["edge_mode_temp_rate_cpuref"])) <= 2e-5


@pytest.mark.parametrize("d,k,edge_prec,node_prec,tol", [(128, 16, "fp16x2", "fp16x2", 2e-5), (128, 8, "fp32", "fp16x2", 2e-5),
                                                       (256, 16, "fp16x2", "fp16x2", 2e-5), (64, 8, "fp16x2", "fp32x3", 2e-5),
                                                       (128, 16, "bf16", "fp16x2", 3e-2)])
def test_model_edge_message_mode_other_precisions(d, k, edge_prec, node_prec, tol):
    """message_source='edge' (the engine's extension: the edge updates are what the nodes aggregate, so every kernel of
    the edge path reaches the outputs) at the f32-accurate precisions and at bf16, against the oracle in that mode."""
    n, nh, L = 400, 2, 3
    snap = synthetic.make_snapshot(n, seed=7 + d + k)
    meta = synthetic.make_metadata()
    g = data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, k, 0.01, 1.0)
    sd = synthetic.make_state_dict(d, d, nh, L, 3)
    m = graph_network.EncodeProcessDecode(d, d, nh, L, 3)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision, m.message_source = edge_prec, node_prec, "edge"
    with torch.no_grad():
        out = m(g)
        ref = cpu_ref.encode_process_decode(sd, g.x.cpu(), g.edge_index.cpu(), g.edge_attr.cpu(), nh, L,
                                            message_source="edge")
    assert rel_err(out["acceleration"].cpu(), ref["acceleration"]) <= tol
    assert rel_err(out["temp_rate"].cpu(), ref["temp_rate"]) <= tol


def test_model_general_edge_order(golden_tiny):
    """Any edge_index is accepted: shuffling the edges takes the atomic aggregation path; same result."""
    g = golden_tiny
    ei = edge_index_from(g)
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(0))
    d = Data(x=torch.from_numpy(g["x"]).to(DEV), edge_index=ei[:, perm].to(DEV),
             edge_attr=torch.from_numpy(g["edge_attr"])[perm].to(DEV))
    with torch.no_grad():
        out = _model(g)(d)
    assert rel_err(out["acceleration"].cpu(), torch.from_numpy(g["acceleration"])) <= TOL
    assert rel_err(out["temp_rate"].cpu(), torch.from_numpy(g["temp_rate"])) <= TOL


def test_model_batched_graphs(golden_tiny):
    g = golden_tiny
    b = Batch.from_data_list([_graph(g), _graph(g)])
    with torch.no_grad():
        out = _model(g)(b)
    want = torch.from_numpy(g["acceleration"])
    assert rel_err(out["acceleration"].cpu(), torch.cat([want, want])) <= TOL


# ------------------------------------------------------------------ graph build + harness vs golden
def test_preprocess_vs_reference_fixture(golden):
    g = golden
    c, e = torch.from_numpy(g["coords"]), torch.from_numpy(g["energy"])
    meta = g["metadata"]
    d = data_utils.preprocess(c[:W].clone(), e[:W].clone(), meta, c[W].clone(), e[W].clone(), 0.0, int(g["k"]),
                              meta["dt"], meta["box_size"])
    assert torch.equal(d.edge_index.cpu(), edge_index_from(g))               # bit exact
    assert torch.equal(d.pos.cpu(), torch.from_numpy(g["pos"]))
    assert torch.equal(d.x.cpu(), torch.from_numpy(g["x"]))                  # one rounding per op, same order
    assert torch.allclose(d.edge_attr.cpu(), torch.from_numpy(g["edge_attr"]), rtol=0, atol=1e-6 * meta["box_size"])
    assert torch.allclose(d.y_acc.cpu(), torch.from_numpy(g["y_acc"]), rtol=1e-6, atol=1e-4)
    assert torch.allclose(d.y_temp_rate.cpu(), torch.from_numpy(g["y_temp_rate"]), rtol=1e-6, atol=1e-5)
    assert d.dt.item() == pytest.approx(meta["dt"]) and d.box_size.item() == pytest.approx(meta["box_size"])


def test_preprocess_noise_uses_reference_rng_stream():
    snap = synthetic.make_snapshot(300, seed=21)
    meta = synthetic.make_metadata()
    c, e = snap["Coordinates"], snap["InternalEnergy"]
    torch.manual_seed(5)
    want = cpu_ref.preprocess(c[:W].clone(), e[:W].clone(), meta, c[W].clone(), e[W].clone(), 3e-4, 8, 0.01, 1.0)
    torch.manual_seed(5)
    got = data_utils.preprocess(c[:W].clone(), e[:W].clone(), meta, c[W].clone(), e[W].clone(), 3e-4, 8, 0.01, 1.0)
    assert torch.allclose(got.pos.cpu(), want["pos"], rtol=0, atol=1e-6)
    assert torch.allclose(got.x.cpu(), want["x"], rtol=0, atol=2e-5)
    assert torch.allclose(got.y_acc.cpu(), want["y_acc"], rtol=1e-5, atol=2e-2)


def test_one_step_harness_vs_reference_fixture(golden):
    g = golden
    snap = dict(Coordinates=torch.from_numpy(g["coords"]), InternalEnergy=torch.from_numpy(g["energy"]))
    res = one_step.validate_one_step(_model(g), snap, g["metadata"], W, DEV, num_neighbors=int(g["k"]),
                                     start_indices=[0])
    assert res["tested_timesteps"] == [W]
    assert res["position_errors"][0] == pytest.approx(float(g["position_mse"]), rel=1e-4)
    assert res["temperature_errors"][0] == pytest.approx(float(g["temperature_mse"]), rel=1e-4)


def _harness_model(h, key):
    m = graph_network.EncodeProcessDecode(int(h["latent"]), int(h["latent"]), int(h["nh"]), int(h["steps"]), 3)
    m.load_state_dict(h[key])
    return m.to(DEV).eval()


def test_one_step_harness_vs_reference_driver(harness):
    """Numbers produced by the reference's own ``validate_one_step`` (one_step_test.py:26-124, run behind an h5py
    stand-in by oracle/make_golden.py): same frames, per-frame MSEs and averages."""
    h = harness
    W1 = int(h["one_step_window"])
    snap = dict(Coordinates=torch.from_numpy(h["coords"]), InternalEnergy=torch.from_numpy(h["energy"]))
    tested = [int(t) for t in h["one_step_tested"]]
    res = one_step.validate_one_step(_harness_model(h, "state_dict_one_step"), snap, h["metadata"], W1, DEV,
                                     num_neighbors=int(h["k"]), start_indices=[t - W1 for t in tested])
    assert res["tested_timesteps"] == tested
    assert res["position_errors"] == pytest.approx(list(h["one_step_position_errors"]), rel=1e-5)
    assert res["temperature_errors"] == pytest.approx(list(h["one_step_temperature_errors"]), rel=1e-5)
    assert res["position_error"] == pytest.approx(float(h["one_step_position_error"]), rel=1e-5)
    # the reference draws its frames with np.random.choice: same seed -> same frames here
    np.random.seed(2024)
    res2 = one_step.validate_one_step(_harness_model(h, "state_dict_one_step"), snap, h["metadata"], W1, DEV,
                                      num_neighbors=int(h["k"]), num_timesteps=3)
    assert res2["tested_timesteps"] == tested


def test_batched_forward_and_momentum_vs_reference_driver(harness):
    """Ragged three-graph batch: forward of the reference model on ``Batch.from_data_list`` and the reference's
    ``momentum_conservation_loss`` (validation.py:5-16) -- reference-produced numbers."""
    h = harness
    meta, kb = h["metadata"], int(h["batch_k"])
    sizes = [int(v) for v in h["batch_sizes"]]
    graphs = []
    for i in range(len(sizes)):
        c, e = torch.from_numpy(h[f"batch_coords{i}"]), torch.from_numpy(h[f"batch_energy{i}"])
        graphs.append(data_utils.preprocess(c[:W].clone(), e[:W].clone(), meta, c[W].clone(), e[W].clone(), 0.0, kb,
                                            meta["dt"], meta["box_size"]))
    b = Batch.from_data_list(graphs)
    assert b.num_graphs == 3 and b.batch.shape[0] == sum(sizes)
    want_acc = torch.from_numpy(h["batch_acceleration"])
    with torch.no_grad():
        acc = _harness_model(h, "state_dict_one_step")(b)["acceleration"]
    assert rel_err(acc.cpu(), want_acc) <= TOL
    w, want = float(h["momentum_weight"]), float(h["batch_momentum"])
    got = float(losses.momentum_conservation_loss(want_acc.to(DEV), b, meta["dt"], w))
    assert abs(got - want) <= 1e-6 * abs(want)                       # the term itself: 1e-6 (north star)
    got2 = float(losses.momentum_conservation_loss(acc, b, meta["dt"], w))
    assert abs(got2 - want) <= 1e-4 * abs(want)                      # fed with the engine's own predictions


def test_on_device_rollout_vs_reference_driver(harness):
    """Trajectory produced by the reference's own ``rollout`` (render_rollout.py:26-90): 3 autoregressive steps."""
    from cosmology_gnn_simulation_amd import rollout as ro
    h = harness
    meta = h["metadata"]
    Wr, R, n = int(h["rollout_window"]), int(h["rollout_steps"]), int(h["n"])
    data = dict(Coordinates=torch.from_numpy(h["coords"])[:Wr + R], InternalEnergy=torch.from_numpy(h["energy"])[:Wr + R])
    m = _harness_model(h, "state_dict_rollout")
    got = ro.rollout(m, data, meta, 0.0, meta["dt"], meta["box_size"], window_size=Wr)
    want_p, want_t = torch.from_numpy(h["rollout_coords"]), torch.from_numpy(h["rollout_energy"])
    assert got["Coordinates"].shape == (Wr + R, n, 3) and got["InternalEnergy"].shape == (Wr + R, n, 1)
    dp = (got["Coordinates"].cpu() - want_p).abs()
    dp = torch.minimum(dp, meta["box_size"] - dp)                    # periodic distance
    assert float(dp.max()) <= 1e-5 * meta["box_size"]
    assert torch.allclose(got["InternalEnergy"].cpu(), want_t, rtol=0, atol=1e-5)
    # the reference builds rollout graphs WITHOUT noise whatever noise_std says (render_rollout.py:44-52)
    noisy = ro.rollout(m, data, meta, 0.1, meta["dt"], meta["box_size"], window_size=Wr)
    assert torch.equal(noisy["Coordinates"], got["Coordinates"]) and torch.equal(noisy["InternalEnergy"], got["InternalEnergy"])
    # no host round trip inside a step.  With the inputs on the device and the weights packed (the calls
    # above), a whole rollout must run without a single device synchronisation.
    dev_data = {k_: v.to(DEV) for k_, v in data.items()}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = ro.rollout(m, dev_data, meta, 0.0, meta["dt"], meta["box_size"], window_size=Wr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again["Coordinates"], got["Coordinates"])


def test_random_init_matches_reference_rng_order():
    """LazyLinear layers are materialised in the reference's first-forward order, so a seeded random
    initialisation equals the restatement run with the same seed."""
    snap = synthetic.make_snapshot(128, seed=3)
    meta = synthetic.make_metadata()
    d = data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, 8, 0.01, 1.0)
    torch.manual_seed(123)
    m = graph_network.EncodeProcessDecode(32, 32, 2, 2, 3).to(DEV)
    with torch.no_grad():
        out = m(d)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    want = cpu_ref.encode_process_decode(sd, d.x.cpu(), d.edge_index.cpu(), d.edge_attr.cpu(), 2, 2)
    assert rel_err(out["acceleration"].cpu(), want["acceleration"]) <= TOL


def test_locality_sorted_execution_is_bitwise_equivalent():
    """The engine renumbers particles in the k-NN build's spatial order (L2 locality); per-receiver summation
    order is unchanged, so the results must be bit-identical to the unsorted run."""
    snap = synthetic.make_snapshot(5000, seed=31)
    meta = synthetic.make_metadata()
    d = data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, 16, 0.01, 1.0)
    assert sorted(d._cgnn_order.cpu().tolist()) == list(range(5000))
    m = graph_network.EncodeProcessDecode(64, 64, 2, 2, 3)
    m.load_state_dict(synthetic.make_state_dict(64, 64, 2, 2, 3))
    m = m.to(DEV).eval()
    with torch.no_grad():
        a = m.forward_with_latents(d)
        m.locality_sort = False
        b = m.forward_with_latents(d)
    for key in ("acceleration", "temp_rate", "x_latent", "edge_latent"):
        assert torch.equal(a[key], b[key]), key


def _same_edge_stream(a, b, kernel, ctx=None):
    """Node outputs never depend on the edge stream: bit-identical.  Edge latents: the 16-edge one-launch
    kernel repeats the per-round kernel's arithmetic exactly (identical bits); the 32-edge one uses another MFMA shape
    and summation order, so the two bf16 computations agree to bf16 rounding noise."""
    for key in ("acceleration", "temp_rate", "x_latent"):
        assert torch.equal(a[key], b[key]), (key, ctx)
    if kernel == "tile16":
        assert torch.equal(a["edge_latent"], b["edge_latent"]), ctx
    else:
        assert rel_l2(a["edge_latent"], b["edge_latent"]) <= 1e-2, ctx
        import edge_checks as ec
        ec.assert_rows_close(a["edge_latent"], b["edge_latent"], 5e-2, f"one-launch vs per-round edge latents {ctx}")


@pytest.mark.parametrize("kernel", ["tile32w", "tile32", "tile16"])
@pytest.mark.parametrize("n,k,latent,nh,steps", [(5000, 16, 128, 2, 3), (300, 8, 128, 2, 10), (3000, 16, 64, 1, 2),
                                                 (2600, 16, 32, 3, 1), (40000, 16, 128, 2, 2), (777, 8, 64, 2, 5)])
def test_all_rounds_in_one_launch_is_bitwise_equivalent(n, k, latent, nh, steps, kernel):
    """All rounds of the edge stream in one launch (reference data flow: the node stream first, then every edge update
    with the edge tile in registers) against one launch per round, and both against the oracle."""
    snap = synthetic.make_snapshot(n, seed=n)
    meta = synthetic.make_metadata()
    d = data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, k, 0.01, 1.0)
    sd = synthetic.make_state_dict(latent, latent, nh, steps, 3)
    m = graph_network.EncodeProcessDecode(latent, latent, nh, steps, 3)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision, m.edge_stream_kernel = "bf16", "fp32x3", kernel
    with ops.OpTimer() as tm, torch.no_grad():
        a = m.forward_with_latents(d)
    assert "edge_stream" in tm.summary() and "edge_block" not in tm.summary()     # the fused path really ran
    m.fuse_rounds = False
    with ops.OpTimer() as tm, torch.no_grad():
        b = m.forward_with_latents(d)
    assert "edge_block" in tm.summary() and "edge_stream" not in tm.summary()
    _same_edge_stream(a, b, kernel)
    want = cpu_ref.encode_process_decode(sd, d.x.cpu(), d.edge_index.cpu(), d.edge_attr.cpu(), nh, steps,
                                         return_latents=True)
    assert rel_err(a["acceleration"].cpu(), want["acceleration"]) <= TOL
    assert rel_l2(a["edge_latent"].cpu(), want["edge_latent"]) <= 3e-2             # bf16 edge MLP
    m.message_source = "edge"                                                      # nodes read the edges: no fusion
    with ops.OpTimer() as tm, torch.no_grad():
        m(d)
    assert "edge_stream" not in tm.summary()


@pytest.mark.parametrize("kernel", ["tile32w", "tile32", "tile16"])
@pytest.mark.parametrize("seed", range(12))
def test_all_rounds_in_one_launch_random_shapes(seed, kernel):
    """Randomised shapes for the one-launch edge stream (tile counts below, at and above the grid's wave count, odd
    numbers of tiles, 1..12 rounds, 1..3 hidden layers) against one launch per round."""
    rng = np.random.default_rng(1000 + seed)
    latent = int(rng.choice([32, 64, 128]))
    k = int(rng.choice([8, 16]))
    n = int(rng.choice([int(rng.integers(k + 1, 200)), int(rng.integers(200, 6000)), int(rng.integers(30000, 70000))]))
    nh = int(rng.integers(1, 4))
    steps = int(rng.integers(1, 13))
    snap = synthetic.make_snapshot(n, seed=seed)
    meta = synthetic.make_metadata()
    d = data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, k, 0.01, 1.0)
    m = graph_network.EncodeProcessDecode(latent, latent, nh, steps, 3)
    m.load_state_dict(synthetic.make_state_dict(latent, latent, nh, steps, 3, seed=seed + 3))
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision, m.edge_stream_kernel = "bf16", "fp32x3", kernel
    with ops.OpTimer() as tm, torch.no_grad():
        a = m.forward_with_latents(d)
    assert "edge_stream" in tm.summary(), (latent, k, n, nh, steps)
    m.fuse_rounds = False
    with torch.no_grad():
        b = m.forward_with_latents(d)
    _same_edge_stream(a, b, kernel, (latent, k, n, nh, steps))


def test_edge_stream_rejects_what_it_cannot_run():
    d, n, k = 64, 64, 8
    m = graph_network.EncodeProcessDecode(d, d, 2, 2, 3)
    m.load_state_dict(synthetic.make_state_dict(d, d, 2, 2, 3))
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision, m.edge_stream_kernel = "bf16", "fp32x3", "tile16"
    rounds = m._pack(17, 4)["rounds"]
    e = ops.TiledRows.from_rows(torch.zeros(n * k, d, device=DEV))
    src = torch.zeros(n * k, dtype=torch.int32, device=DEV)
    tab = torch.zeros(2, n, d, dtype=torch.bfloat16, device=DEV)
    ops.edge_stream([r.edge for r in rounds], tab, tab, src, src, e)                      # fine
    with pytest.raises(ops.CgnnError, match="rounds"):                                   # table has 2 rounds, 1 given
        ops.edge_stream([rounds[0].edge], tab, tab, src, src, e)
    with pytest.raises(ops.CgnnError, match="bfloat16"):
        ops.edge_stream([r.edge for r in rounds], tab.float(), tab, src, src, e)
    m32 = graph_network.EncodeProcessDecode(d, d, 2, 2, 3)
    m32.load_state_dict(synthetic.make_state_dict(d, d, 2, 2, 3))
    m32 = m32.to(DEV).eval()                                                             # fp32 packing: 32-row kernels
    with pytest.raises(ops.CgnnError, match="bf16_n16"):
        ops.edge_stream([r.edge for r in m32._pack(17, 4)["rounds"]], tab, tab, src, src, e)
    # shapes the fused kernel is not built for fall back to one launch per round inside the model
    big = graph_network.EncodeProcessDecode(256, 256, 2, 1, 3)
    assert not big._can_fuse_rounds([], 256)


def test_on_device_rollout_matches_restatement():
    """render_rollout.rollout counterpart: 3 autoregressive steps on the device vs the oracle's restatement."""
    from cosmology_gnn_simulation_amd import rollout as ro
    n, k, d, L, Wr = 400, 8, 32, 2, 6
    snap = synthetic.make_snapshot(n, window=Wr + 2, seed=51)
    meta = synthetic.make_metadata()
    sd = synthetic.make_state_dict(d, d, 2, L, 3, node_in=3 * (Wr - 1) + Wr)
    m = graph_network.EncodeProcessDecode(d, d, 2, L, 3)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    state = torch.random.get_rng_state()
    got = ro.rollout(m, snap, meta, 0.0, meta["dt"], meta["box_size"], window_size=Wr, num_neighbors=k)
    assert torch.equal(torch.random.get_rng_state(), state)          # reference_rng=False leaves the RNG alone
    want = cpu_ref.rollout(sd, 2, L, snap["Coordinates"], snap["InternalEnergy"], meta, Wr, k, Wr + 3)
    assert got["Coordinates"].shape == (Wr + 3, n, 3) and got["InternalEnergy"].shape == (Wr + 3, n, 1)
    assert torch.equal(got["Coordinates"][:Wr].cpu(), snap["Coordinates"][:Wr])
    dp = (got["Coordinates"].cpu() - want["Coordinates"]).abs()
    dp = torch.minimum(dp, 1.0 - dp)                                 # periodic distance
    assert float(dp.max()) <= 1e-5
    assert torch.allclose(got["InternalEnergy"].cpu(), want["InternalEnergy"], rtol=0, atol=1e-5)
    err = ro.calculate_errors(got, snap)
    assert len(err["position_errors"]) == Wr + 3 and err["position_errors"][0] == 0.0


@pytest.mark.parametrize("d,h,k,nh,L,edge_prec,node_prec", [(256, 256, 32, 2, 2, "bf16", "fp32x3"),      # cfg5 shape
                                                          (256, 256, 8, 2, 1, "fp32", "fp32"),
                                                          (64, 128, 8, 2, 2, "bf16", "fp32"),           # hidden != latent
                                                          (256, 128, 16, 1, 2, "fp32", "fp32x3"),
                                                          (128, 128, 16, 3, 2, "bf16", "fp32x3"),       # 3 hidden layers
                                                          (128, 128, 16, 2, 3, "fp16x2", "fp16x2"),     # cfg2's fast path
                                                          (128, 128, 8, 1, 2, "fp16x2", "fp16x2"),
                                                          (64, 64, 8, 2, 2, "fp16x2", "fp16x2"),        # falls back to f32 edges
                                                          (256, 256, 32, 2, 2, "bf16", "fp16x2"),       # cfg5 preset: 32-row fp16x2 node path
                                                          (256, 128, 16, 1, 2, "fp16x2", "fp16x2"),
                                                          (64, 128, 8, 2, 2, "fp16x2", "fp16x2")])
def test_model_other_shapes_vs_oracle(d, h, k, nh, L, edge_prec, node_prec):
    """Shapes beyond the committed fixtures (README.md:59-62 ranges; BASELINE cfg5 = latent 256, k 32): the HIP
    forward against the oracle on a fresh graph."""
    n = 300
    snap = synthetic.make_snapshot(n, seed=61 + d + k)
    meta = synthetic.make_metadata()
    g = data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, k, 0.01, 1.0)
    sd = synthetic.make_state_dict(d, h, nh, L, 3)
    m = graph_network.EncodeProcessDecode(d, h, nh, L, 3)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision = edge_prec, node_prec
    with torch.no_grad():
        out = m.forward_with_latents(g)
        ref = cpu_ref.encode_process_decode(sd, g.x.cpu(), g.edge_index.cpu(), g.edge_attr.cpu(), nh, L,
                                            return_latents=True)
    assert rel_err(out["acceleration"].cpu(), ref["acceleration"]) <= TOL
    assert rel_err(out["temp_rate"].cpu(), ref["temp_rate"]) <= TOL
    assert rel_l2(out["edge_latent"].cpu(), ref["edge_latent"]) <= (3e-2 if edge_prec == "bf16" else TOL)
    if edge_prec != "bf16":
        assert rel_err(out["edge_latent"].cpu(), ref["edge_latent"]) <= TOL


def test_hip_graph_replay_equals_eager(golden_tiny):
    """The captured launch sequence (HIP graph) reproduces the eager forward bit for bit, also for new inputs."""
    from cosmology_gnn_simulation_amd.graphed import GraphedForward
    g = golden_tiny
    m = _model(g, edge_precision="bf16", node_precision="fp32x3")
    d = _graph(g)
    with torch.no_grad():
        eager = m(d)
    gf = GraphedForward(m, d)
    out = gf()
    assert torch.equal(out["acceleration"], eager["acceleration"]) and torch.equal(out["temp_rate"], eager["temp_rate"])
    x2 = d.x * 0.5
    d2 = Data(x=x2, edge_index=d.edge_index, edge_attr=d.edge_attr)
    with torch.no_grad():
        eager2 = m(d2)
    out2 = gf(x2)
    assert torch.equal(out2["acceleration"], eager2["acceleration"])


@pytest.mark.parametrize("edge_prec,node_prec", [("bf16", "fp16x2"), ("fp16x2", "fp16x2")])
def test_hip_graph_replay_at_a_size_that_takes_the_lds_resident_and_planned_paths(edge_prec, node_prec):
    """Above 4096 / 8192 rows the forward uses kernels that set launch attributes (dynamic LDS for resident weights, ring
    kernels) and the per-graph aggregation plan: capture and replay must still equal the eager forward bit for bit."""
    from cosmology_gnn_simulation_amd.graphed import GraphedForward
    n, k, d, nh, L = 9000, 16, 128, 2, 3
    snap = synthetic.make_snapshot(n, seed=3)
    meta = synthetic.make_metadata()
    g = data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, k, 0.01, 1.0)
    m = graph_network.EncodeProcessDecode(d, d, nh, L, 3)
    m.load_state_dict(synthetic.make_state_dict(d, d, nh, L, 3))
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision = edge_prec, node_prec
    with torch.no_grad():
        eager = m(g)
    gf = GraphedForward(m, g)
    out = gf()
    assert torch.equal(out["acceleration"], eager["acceleration"]) and torch.equal(out["temp_rate"], eager["temp_rate"])
    x2 = g.x * 0.5
    with torch.no_grad():
        eager2 = m(Data(x=x2, edge_index=g.edge_index, edge_attr=g.edge_attr))
    out2 = gf(x2)
    assert torch.equal(out2["acceleration"], eager2["acceleration"]) and torch.equal(out2["temp_rate"], eager2["temp_rate"])


def test_large_ragged_batch_equals_its_members():
    """train.py:247 / validation.py:56 batch several graphs: a three-graph batch big enough for the planned aggregation,
    the ring kernels and the LDS-resident weights gives every member exactly what it gets alone (rows are independent
    and every receiver sums its neighbours in the same order)."""
    k, d, nh, L = 16, 128, 2, 2
    meta = synthetic.make_metadata()
    graphs = []
    for i, n in enumerate((3000, 5000, 2500)):
        snap = synthetic.make_snapshot(n, seed=20 + i)
        graphs.append(data_utils.preprocess(snap["Coordinates"][:W], snap["InternalEnergy"][:W], meta, None, None, 0.0, k,
                                            0.01, 1.0))
    m = graph_network.EncodeProcessDecode(d, d, nh, L, 3)
    m.load_state_dict(synthetic.make_state_dict(d, d, nh, L, 3))
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision = "bf16", "fp16x2"
    with torch.no_grad():
        alone = [m(g) for g in graphs]
        out = m(Batch.from_data_list(graphs))
    for key in ("acceleration", "temp_rate"):
        assert torch.equal(out[key], torch.cat([a[key] for a in alone])), key


def test_fixed_k_hint_is_bound_to_its_edge_index(golden_tiny):
    """A caller that reorders the edges of a preprocessed graph (same size, no longer receiver-sorted) must get the
    general path, not the fixed-k kernels on a stale hint: results equal the oracle on the reordered list."""
    g = golden_tiny
    c, e = torch.from_numpy(g["coords"]), torch.from_numpy(g["energy"])
    d = data_utils.preprocess(c[:W].clone(), e[:W].clone(), g["metadata"], None, None, 0.0, int(g["k"]), g["metadata"]["dt"],
                              g["metadata"]["box_size"])
    m = _model(g)
    with torch.no_grad():
        want = m(d)
    perm = torch.randperm(d.edge_index.shape[1], generator=torch.Generator().manual_seed(0)).to(DEV)
    d.edge_index = d.edge_index[:, perm].contiguous()        # same shape, shuffled order; the hint object is still there
    d.edge_attr = d.edge_attr[perm].contiguous()
    assert getattr(d, "_cgnn_fixed_k", None) == int(g["k"])
    with torch.no_grad():
        got = m(d)
    assert rel_err(got["acceleration"], want["acceleration"]) <= TOL      # sums in another order, same values
    src, dst, fk = graph_network._graph_arrays(d, d.x.shape[0])
    assert fk == 0


def test_invalidate_packed_after_a_data_update(golden_tiny):
    g = golden_tiny
    m = _model(g)
    with torch.no_grad():
        a = m(_graph(g))
        for p_ in m.parameters():
            p_.data.mul_(0.5)                    # does not bump the parameter's version counter
        m.invalidate_packed()
        b = m(_graph(g))
    sd = {k_: v * 0.5 for k_, v in g["state_dict"].items()}
    want = cpu_ref.encode_process_decode(sd, torch.from_numpy(g["x"]), edge_index_from(g), torch.from_numpy(g["edge_attr"]),
                                         int(g["nh"]), int(g["steps"]))
    assert rel_err(b["acceleration"].cpu(), want["acceleration"]) <= TOL
    assert not torch.equal(a["acceleration"], b["acceleration"])
