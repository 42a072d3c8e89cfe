"""GPU: cgnn_mlp_rows / cgnn_mlp_rows_project with CGNN_F16X2_N16 weights -- the node encoder and the decoders on the
two-waves-per-SIMD ring kernel (csrc/mlp_rows_f2.hip) -- against a float64 torch evaluation, with the gates the
project holds this arithmetic to elsewhere (test_gpu_node_block.py, test_gpu_parity.py):

    max |got - want| <= 2e-6 max |want|      and      rel-L2 <= 2e-6        (no element left out)

Inputs are seeded normal, weights and biases seeded uniform in +-1/sqrt(fan_in).  The projection epilogue is compared
with ops.project_nodes of the same rows in the same table format: both round the same f32-accurate sums once to the
table's type, so they differ by at most one unit of that rounding (2^-10 relative for fp16, 2^-7 for bf16) plus the
f32 summation-order noise near zero (1e-5 of the table's largest value)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, rel_l2
from cosmology_gnn_simulation_amd import _lib, data_utils, graph_network, ops, synthetic
from cosmology_gnn_simulation_amd._lib import CgnnError
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS = (1, 15, 16, 17, 127, 128, 129, 389, 4133)     # one row, wave tile edge, workgroup step edge, several steps, many ring wraps
GATE = 2e-6
SENTINEL = -12345.0


def _rand_mlp(seed, dims, ln):
    gen = torch.Generator().manual_seed(seed)
    lin = []
    for i in range(len(dims) - 1):
        bound = 1.0 / np.sqrt(dims[i])
        w = (torch.rand(dims[i + 1], dims[i], generator=gen) * 2 - 1) * bound
        b = (torch.rand(dims[i + 1], generator=gen) * 2 - 1) * bound
        lin.append((w.to(DEV), b.to(DEV)))
    lnp = None
    if ln:
        lnp = ((1 + 0.1 * torch.randn(dims[-1], generator=gen)).to(DEV), (0.1 * torch.randn(dims[-1], generator=gen)).to(DEV))
    return lin, lnp


def _f64(lin, lnp, x):
    h = x.double()
    for i, (w, b) in enumerate(lin):
        h = h @ w.double().t() + b.double()
        if i < len(lin) - 1:
            h = torch.relu(h)
    if lnp is not None:
        h = F.layer_norm(h, (h.shape[1],), lnp[0].double(), lnp[1].double(), 1e-5)
    return h


def _encoder(seed, fin, nh):
    lin, lnp = _rand_mlp(seed, [fin] + [128] * nh + [128], True)
    return lin, lnp, ops.PackedMLP(lin, lnp, "fp16x2_n16")


def _decoder(seed, fout, nh):
    lin, _ = _rand_mlp(seed, [128] * (nh + 1) + [fout], False)
    return lin, ops.PackedMLP(lin, None, "fp16x2_n16")


def _inputs(seed, n, width):
    return torch.randn(n, width, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _gate(got, want, what):
    got, want = got.double(), want.double()
    linf = float((got - want).abs().max() / want.abs().max())
    l2 = float((got - want).norm() / want.norm())
    print(f"{what}: max-abs/max-abs {linf:.3e}  rel-L2 {l2:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert linf <= GATE and l2 <= GATE, (what, linf, l2)


# ------------------------------------------------------------------ 1. encoder
@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("fin", [4, 17, 32])
def test_encoder_meets_the_f32_gate(fin, nh):
    lin, lnp, mlp = _encoder(100 * fin + nh, fin, nh)
    for n in NS:
        x = _inputs(n + fin, n, fin)
        got = ops.mlp_rows(mlp, x)
        torch.cuda.synchronize()
        assert got.shape == (n, 128)
        _gate(got, _f64(lin, lnp, x), f"encoder fin={fin} nh={nh} n={n}")


def test_encoder_reads_rows_with_a_stride():
    fin, nh, n = 17, 2, 389
    lin, lnp, mlp = _encoder(7, fin, nh)
    wide = _inputs(8, n, fin + 6)
    x = wide[:, 3:3 + fin]                           # ld_x = 23 > 17, rows start at an odd float
    assert x.stride(0) == fin + 6
    _gate(ops.mlp_rows(mlp, x), _f64(lin, lnp, x), "encoder ld_x=23")


# ------------------------------------------------------------------ 2. decoder
@pytest.mark.parametrize("nh", [1, 2, 3])
@pytest.mark.parametrize("fout", [1, 3, 16])
def test_decoder_meets_the_f32_gate_and_writes_nothing_else(fout, nh):
    lin, mlp = _decoder(200 * fout + nh, fout, nh)
    for n in NS:
        x = _inputs(n + fout, n, 128)
        buf = torch.full((n + 3, fout + 5), SENTINEL, device=DEV)
        out = buf[:n, :fout]                         # ld_y = fout + 5
        ops.mlp_rows(mlp, x, out=out)
        torch.cuda.synchronize()
        _gate(out, _f64(lin, None, x), f"decoder fout={fout} nh={nh} n={n}")
        assert bool((buf[n:] == SENTINEL).all()) and bool((buf[:, fout:] == SENTINEL).all()), (fout, nh, n)


# ------------------------------------------------------------------ 3. position independence
def test_a_rows_result_does_not_depend_on_its_position():
    n = 4133
    _, _, enc = _encoder(1, 17, 2)
    _, dec = _decoder(2, 3, 2)
    for mlp, width in ((enc, 17), (dec, 128)):
        x = _inputs(3, n, width)
        whole = ops.mlp_rows(mlp, x)
        parts, a = [], 0
        for size in (2000, 77, 2000, 56):            # slices of 2000 rows and of 77 rows (and the 56 that remain)
            parts.append(ops.mlp_rows(mlp, x[a:a + size]))
            a += size
        assert a == n
        assert torch.equal(whole, torch.cat(parts))


# ------------------------------------------------------------------ 4. repeatability
def test_the_same_call_gives_the_same_bits():
    n = 4133
    _, _, enc = _encoder(1, 17, 2)
    _, dec = _decoder(2, 3, 2)
    for mlp, width in ((enc, 17), (dec, 128)):
        x = _inputs(4, n, width)
        first = ops.mlp_rows(mlp, x).clone()
        for _ in range(2):
            assert torch.equal(ops.mlp_rows(mlp, x), first)


# ------------------------------------------------------------------ 5. range contract
def test_an_activation_beyond_fp16_turns_its_own_row_non_finite_and_no_other():
    n, bad = 389, 137
    _, _, enc = _encoder(1, 17, 2)
    _, dec = _decoder(2, 3, 2)
    for mlp, width in ((enc, 17), (dec, 128)):
        x = _inputs(5, n, width)
        clean = ops.mlp_rows(mlp, x)
        x2 = x.clone()
        x2[bad, 5] = 7e4
        got = ops.mlp_rows(mlp, x2)
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(got[bad]).any())
        keep = torch.arange(n, device=DEV) != bad
        assert bool(torch.isfinite(clean).all()) and torch.equal(got[keep], clean[keep])


# ------------------------------------------------------------------ 6. fused projection
@pytest.mark.parametrize("fmt,unit", [(_lib.P_F16_S32, 2.0 ** -10), (_lib.P_BF16_S32, 2.0 ** -7), (_lib.P_BF16_S16, 2.0 ** -7)])
def test_projection_epilogue_writes_project_nodes_tables(fmt, unit):
    fin, nh = 17, 2
    _, _, enc = _encoder(11, fin, nh)
    gen = torch.Generator().manual_seed(12)
    bound = 1.0 / np.sqrt(384)
    w1 = ((torch.rand(128, 384, generator=gen) * 2 - 1) * bound).to(DEV)          # [Ws | Wd | We] of an edge model
    b1 = ((torch.rand(128, generator=gen) * 2 - 1) * bound).to(DEV)
    ws, wd = ops.PackedLinear(w1, None, "bf16", 0, 128), ops.PackedLinear(w1, b1, "bf16", 128, 128)
    ws16, wd16 = ops.PackedLinear(w1, None, "bf16_n16", 0, 128), ops.PackedLinear(w1, b1, "bf16_n16", 128, 128)
    pdt = ops.p_format_dtype(fmt)
    for n in (16, 129, 4133):
        x = _inputs(n, n, fin)
        plain = ops.mlp_rows(enc, x)
        ps_buf = torch.full((n + 4, 128), 3.0, dtype=pdt, device=DEV)
        pd_buf = torch.full((n + 4, 128), 3.0, dtype=pdt, device=DEV)
        fused = ops.mlp_rows(enc, x, next_projection=(ws16, wd16, ps_buf[:n], pd_buf[:n], fmt))
        torch.cuda.synchronize()
        assert torch.equal(fused, plain)
        want_ps, want_pd = ops.project_nodes(ws, wd, plain, p_format=fmt)
        for name, got, want in (("ps", ps_buf, want_ps), ("pd", pd_buf, want_pd)):
            a, b = got[:n].double(), want.double()
            excess = (a - b).abs() - (unit * torch.maximum(a.abs(), b.abs()) + 1e-5 * b.abs().max())
            print(f"{name} fmt={fmt} n={n}: max |a-b| {float((a - b).abs().max()):.3e}, worst excess {float(excess.max()):.3e}, "
                  f"differing {int((a != b).sum())} of {a.numel()}")
            assert bool(torch.isfinite(a).all()) and float(excess.max()) <= 0.0, (name, fmt, n)
            assert bool((got[n:] == 3.0).all()), (name, fmt, n)


# ------------------------------------------------------------------ 7. row index
def test_row_index_reads_and_writes_permuted_rows():
    n = 4133
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(6)).to(DEV).int()
    _, _, enc = _encoder(1, 17, 2)
    x = _inputs(7, n, 17)
    assert torch.equal(ops.mlp_rows(enc, x, index=perm), ops.mlp_rows(enc, x[perm.long()].contiguous()))
    _, dec = _decoder(2, 3, 2)
    h = _inputs(8, n, 128)
    plain = ops.mlp_rows(dec, h)
    want = torch.empty_like(plain)
    want[perm.long()] = plain
    assert torch.equal(ops.mlp_rows(dec, h, index=perm), want)


# ------------------------------------------------------------------ 8-10. the model
@pytest.fixture(scope="module")
def small_model():
    n, k, d, nh, L = 1000, 8, 128, 2, 2
    snap = synthetic.make_snapshot(n, seed=21)
    meta = synthetic.make_metadata()
    g = data_utils.preprocess(snap["Coordinates"][:5], snap["InternalEnergy"][:5], meta, None, None, 0.0, k, meta["dt"],
                              meta["box_size"], device=torch.device(DEV))
    sd = synthetic.make_state_dict(d, d, nh, L, 3)
    m = graph_network.EncodeProcessDecode(d, d, nh, L, 3)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.edge_precision, m.node_precision = "bf16", "fp16x2"
    with torch.no_grad():
        ref = cpu_ref.encode_process_decode(sd, g.x.cpu(), g.edge_index.cpu(), g.edge_attr.cpu(), nh, L)
    return m, g, ref


def test_model_runs_three_mlp_rows_one_gather_and_no_project_nodes(small_model):
    m, g, _ = small_model
    assert getattr(g, "_cgnn_order", None) is not None              # the locality order exists
    with torch.no_grad():
        m(g)
        with ops.OpTimer() as tm:
            m(g)
    summ = tm.summary()
    print({k: v[0] for k, v in summ.items()})
    assert summ["mlp_rows"][0] == 3 and "project_nodes" not in summ and summ["gather_rows"][0] == 1


def test_model_fused_projection_against_the_unfused_path(small_model):
    m, g, _ = small_model
    with torch.no_grad():
        on = m.forward_with_latents(g)
        m.fuse_encoder_projection = False
        try:
            with ops.OpTimer() as tm:
                off = m.forward_with_latents(g)
        finally:
            m.fuse_encoder_projection = True
    assert tm.summary()["project_nodes"][0] == 1
    for key in ("acceleration", "temp_rate", "x_latent"):
        assert torch.equal(on[key], off[key]), key
    e = rel_l2(on["edge_latent"].cpu(), off["edge_latent"].cpu())
    print(f"edge latents, fused against unfused round-0 tables: rel-L2 {e:.3e}")
    assert e <= 1e-2


def test_model_outputs_meet_the_fp32_gate(small_model):
    m, g, ref = small_model
    with torch.no_grad():
        out = m(g)
    for key in ("acceleration", "temp_rate"):
        e = rel_err(out[key].cpu(), ref[key])
        print(f"{key}: rel err {e:.3e}")
        assert e <= 1e-5, key


# ------------------------------------------------------------------ 11. refusal
@pytest.mark.parametrize("dims,ln", [([17, 64, 64, 64], True), ([17, 128, 128, 128, 128, 128], True),
                                     ([128, 64, 64, 3], False), ([128, 128, 128, 128, 128, 3], False)])
def test_unsupported_shapes_are_refused(dims, ln):
    lin, lnp = _rand_mlp(1, dims, ln)
    mlp = ops.PackedMLP(lin, lnp, "fp16x2_n16")
    x = _inputs(1, 40, dims[0])
    out = torch.full((40, dims[-1]), SENTINEL, device=DEV)
    with pytest.raises(CgnnError):
        ops.mlp_rows(mlp, x, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())             # nothing was launched
