"""GPU: every per-call bf16 kernel against an emulation of its arithmetic (oracle/bf16_stream.py: emulate_project,
emulate_edge_update, emulate_encoder), gated per element / per row (tests/edge_checks.py; the gates themselves are tested
on the CPU in test_bf16_kernel_gates_cpu.py).  test_gpu_parity.py holds the same kernels to one relative L2 norm of 3e-2
against the f32 oracle, which a dropped bias or LayerNorm vector passes.

Gates
* tables (Ps / Pd): every element is the correctly rounded value of some f32 evaluation of its sum
  (assert_table_is_rounded_exact: no tuned number), decoded with the layout maps restated from include/cgnn.h;
* updates u (``e_upd``, or ``e_out`` with residual = 0), EVERY row: max-abs <= 1e-2 x scale, rel-L2 <= 2e-3, per-row
  relative norm <= 1e-2; ``e_out`` element-wise within 2^-22 max(|e_in|, |u|) of e_in + u.
* A tighter measured rel-L2 gate does not fit: float64-sum emulation against float32-matmul emulation (reference against
  reference) measures up to 9.3e-5 .. 1.6e-4 on u over these shapes (seed dependent), times 10 = 1.6e-3, above half (1.5e-3) of what truncated
  activations cost (3.0e-3 .. 3.3e-3 on u).  The 2e-3 stands alone; on u it rejects truncation (edge_checks.py).

Inputs are seeded: weights and biases uniform +-1/sqrt(fan_in), gamma 1 +- 0.1, beta +- 0.1, x = 3 randn with 50 rows
scaled by 1e-3 and 50 by 30, e = 3 randn.  For the edge kernels Ps / Pd are built in Python (bf16-representable random
values laid out with logical_to_table): their read side does not depend on cgnn_project_nodes; one chained case per
family takes its tables from the kernel.

Case -> compiled instantiation (dispatch in csrc/mlp_rows.hip, edge_block.hip, edge_block_ring256.hip)
* test_project_nodes_tables: project_kernel<CGNN_BF16, {P_BF16_S32, P_BF16_S16}, D/32, H/32, WLDS> for the six (H, D) of
  CGNN_FOR_EACH_PAIR, <CGNN_BF16, P_F16_S32, 4, 4, WLDS>; WLDS = false for n < 4096, true from 4096 where both matrices
  fit (all but 256 x 256: global weights at every n); ps-only and pd-only calls take the nullptr branches.
* test_projection_epilogues: node_block_n16 (fp32x3_n16) and node_block_f2 (fp16x2_n16) epilogues, mlp_rows_f2.hip's
  epilogue, each in the three table formats; n = 16, 129 (remainder launch), 4133 (whole steps + remainder).
* test_edge_block_bf16[H-D]: edge_block_kernel<CGNN_BF16, false, H/32, D/32> at 1, 33, 4095 edges (and always at
  256-wide shapes); edge_block_lds_kernel<H/32, D/32> at 4096, 4101 edges where hidden, latent <= 128.
* test_edge_block_bf16_n16[H-D]: edge_block_n16_kernel<H/32, D/32, 1024, false> (no fused aggregation) for (32,32),
  (64,64), (128,128), (128,64); 1..3 hidden layers are a run-time loop.
* test_edge_block_ring256: edge_block_ring256_kernel<NH, RAGGED> for NH = 1, 2, 3: E = 32 -> <NH, true> alone; 100, 128 ->
  <NH, false> alone (one step); 539 -> <NH, false> (4 steps) + <NH, true> (2 half tiles); 80069 -> <NH, false> with 625
  steps on a grid of at most one workgroup per CU (256) + <NH, true> with 6 half tiles, the last tile partial.
* test_edge_encoders_bf16[H-D]: mlp_rows_kernel<CGNN_BF16, WLDS, 1, H/32, D/32> tiled and row-major (full and ragged
  stores), WLDS = true at 4099 rows where H, D <= 128.
* test_edge_encoders_bf16_n16[H-D]: edge_encode_n16_kernel<H/32, D/32> for the four pairs above.
residual = 0 / 1 and e_upd given / NULL are run-time branches of every edge kernel: all four run in every case.

Worst values seen on an MI355X are in DESIGN.md (verification); every test prints its own (``pytest -s``)."""
import pytest
import torch

import edge_checks as ec
from cosmology_gnn_simulation_amd import _lib, ops
from cosmology_gnn_simulation_amd._lib import CgnnError
from oracle import bf16_stream as bs

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMATS = {"s32": _lib.P_BF16_S32, "s16": _lib.P_BF16_S16, "f16": _lib.P_F16_S32}
assert (_lib.P_BF16_S32, _lib.P_BF16_S16, _lib.P_F16_S32) == (bs.P_BF16_S32, bs.P_BF16_S16, bs.P_F16_S32)
N16_PAIRS = [(32, 32), (64, 64), (128, 128), (128, 64)]
FILL = 3.0


def _dev(t):
    if isinstance(t, (list, tuple)):
        return type(t)(_dev(v) for v in t)
    return None if t is None else t.to(DEV)


class _Worst:
    """Largest figures seen by one test, printed at its end."""

    def __init__(self, what):
        self.what, self.st, self.cases = what, {}, 0

    def add(self, st):
        self.cases += 1
        for k, v in st.items():
            self.st[k] = max(self.st.get(k, 0.0), v)

    def report(self):
        print(f"{self.what}: {self.cases} gated matrices, worst " + ", ".join(f"{k} {v:.2e}" for k, v in self.st.items()))


def _gate_tables(name, fmt, ps, pd, x, ws, wd, b1, n, counts):
    """Both tables ([n + 4, H] buffers, the first n rows written) against emulate_project of the f32 rows ``x``."""
    dtype = bs.P_FORMAT_DTYPE[fmt]
    for which, buf, w, b in (("ps", ps, ws, None), ("pd", pd, wd, b1)):
        if buf is None:
            continue
        exact, bound = bs.emulate_project(x, w, b, dtype)
        differ = ec.assert_table_is_rounded_exact(bs.table_to_logical(buf[:n], fmt), exact, bound, dtype, f"{name} {which} n={n}")
        assert bool((buf[n:] == FILL).all()), f"{name} {which} n={n}: rows past n were written"
        counts[0] += differ
        counts[1] += exact.numel()


# ------------------------------------------------------------------ a. cgnn_project_nodes
@pytest.mark.parametrize("fmt", ["s32", "s16", "f16"])
def test_project_nodes_tables(fmt):
    p_format = FORMATS[fmt]
    dtype = bs.P_FORMAT_DTYPE[p_format]
    counts = [0, 0]
    for hidden, latent in (ec.PAIRS if fmt != "f16" else [(128, 128)]):
        xs, ws, wd, b1 = _dev(ec.projection_problem(hidden + latent, hidden, latent, 4133))
        pws, pwd = ops.PackedLinear(ws, None, "bf16"), ops.PackedLinear(wd, b1, "bf16")
        for n in (1, 31, 32, 33, 4095, 4096, 4133):          # 4096: the matrices move into LDS
            x = xs[4133 - n:].contiguous() if n < 200 else xs[:n].contiguous()      # (from 200 rows on: the scaled blocks)
            bufs = [torch.full((n + 4, hidden), FILL, dtype=dtype, device=DEV) for _ in range(4)]
            ops.project_nodes(pws, pwd, x, bufs[0][:n], bufs[1][:n], p_format)
            ops.project_nodes(pws, None, x, bufs[2][:n], None, p_format)
            ops.project_nodes(None, pwd, x, None, bufs[3][:n], p_format)
            torch.cuda.synchronize()
            name = f"project_nodes {fmt} ({hidden},{latent})"
            _gate_tables(name, p_format, bufs[0], bufs[1], x, ws, wd, b1, n, counts)
            assert torch.equal(bufs[2], bufs[0]) and torch.equal(bufs[3], bufs[1]), (name, n)       # ps alone, pd alone
    print(f"project_nodes {fmt}: {counts[0]} of {counts[1]} elements differ from the float64-rounded value, all inside the f32 bound")


def test_project_nodes_refuses_what_it_has_no_kernel_for():
    for hidden, latent in [p for p in ec.PAIRS if p != (128, 128)] + [(256, 128)]:
        x, ws, wd, b1 = _dev(ec.projection_problem(1, hidden, latent, 40))
        pws, pwd = ops.PackedLinear(ws, None, "bf16"), ops.PackedLinear(wd, b1, "bf16")
        formats = ["f16"] if (hidden, latent) in ec.PAIRS else ["s32", "s16", "f16"]      # (256, 128) is no compiled pair
        for fmt in formats:
            dtype = bs.P_FORMAT_DTYPE[FORMATS[fmt]]
            ps = torch.full((40, hidden), FILL, dtype=dtype, device=DEV)
            pd = torch.full((40, hidden), FILL, dtype=dtype, device=DEV)
            with pytest.raises(CgnnError):
                ops.project_nodes(pws, pwd, x, ps, pd, FORMATS[fmt])
            torch.cuda.synchronize()
            assert bool((ps == FILL).all()) and bool((pd == FILL).all()), (hidden, latent, fmt)


# ------------------------------------------------------------------ b. projection epilogues
@pytest.mark.parametrize("fmt", ["s32", "s16", "f16"])
def test_projection_epilogues(fmt):
    """The tables the node kernels and the encoder write from their registers, against emulate_project of the f32 rows the
    same call returned (until now they were compared with cgnn_project_nodes only)."""
    p_format, d = FORMATS[fmt], 128
    dtype = bs.P_FORMAT_DTYPE[p_format]
    gen = torch.Generator().manual_seed(31)
    w1e, b1e = _dev(ec.rand_linear(gen, d, 3 * d))
    ws, wd = w1e[:, :d].contiguous(), w1e[:, d:2 * d].contiguous()
    ws16, wd16 = ops.PackedLinear(ws, None, "bf16_n16"), ops.PackedLinear(wd, b1e, "bf16_n16")
    node = _dev([ec.rand_linear(gen, d, 2 * d), ec.rand_linear(gen, d, d), ec.rand_linear(gen, d, d)])
    node_ln = _dev(ec.rand_layer_norm(gen, d))
    enc = _dev([ec.rand_linear(gen, d, 17), ec.rand_linear(gen, d, d), ec.rand_linear(gen, d, d)])
    enc_ln = _dev(ec.rand_layer_norm(gen, d))
    xs, aggs, feats = _dev(ec.node_rows(gen, 4133, d)), _dev(4 * torch.randn(4133, d, generator=gen)), _dev(torch.randn(4133, 17, generator=gen))
    counts = [0, 0]
    for n in (16, 129, 4133):
        def tables():
            return (torch.full((n + 4, d), FILL, dtype=dtype, device=DEV), torch.full((n + 4, d), FILL, dtype=dtype, device=DEV))
        for prec in ("fp32x3_n16", "fp16x2_n16"):
            w1, b1 = node[0]
            wx, wa = ops.PackedLinear(w1, b1, prec, 0, d), ops.PackedLinear(w1, None, prec, d, d)
            mlp = ops.PackedMLP([(w1[:, :d].contiguous(), None)] + node[1:], node_ln, prec)
            ps, pd = tables()
            rows = ops.node_block(mlp, wx, wa, xs[:n].contiguous(), aggs[:n].contiguous(), None, True, (ws16, wd16, ps[:n], pd[:n], p_format))
            torch.cuda.synchronize()
            _gate_tables(f"node_block {prec} epilogue {fmt}", p_format, ps, pd, rows, ws, wd, b1e, n, counts)
        mlp = ops.PackedMLP(enc, enc_ln, "fp16x2_n16")
        ps, pd = tables()
        rows = ops.mlp_rows(mlp, feats[:n].contiguous(), next_projection=(ws16, wd16, ps[:n], pd[:n], p_format))
        torch.cuda.synchronize()
        _gate_tables(f"mlp_rows fp16x2_n16 epilogue {fmt}", p_format, ps, pd, rows, ws, wd, b1e, n, counts)
    print(f"projection epilogues {fmt}: {counts[0]} of {counts[1]} elements differ from the float64-rounded value, all inside the f32 bound")


# ------------------------------------------------------------------ c. cgnn_edge_block
def _edge_case(worst, prec, p_format, p, what, packed=None, l2_gate=None, alias=False, tables=None):
    """One problem through cgnn_edge_block with residual 1 / 0 and e_upd given / NULL; u against emulate_edge_update."""
    q = {k: _dev(v) for k, v in p.items()}
    mlp = packed or ops.PackedMLP([(q["lins"][0][0], None)] + list(q["lins"][1:]), q["ln"], prec)
    if tables is None:
        tps, tpd = bs.logical_to_table(q["ps"], p_format), bs.logical_to_table(q["pd"], p_format)
    else:
        tps, tpd = tables
    want = bs.emulate_edge_update(q["ps"], q["pd"], q["src"], q["dst"], q["e"], q["lins"], q["ln"])
    e_in = ops.TiledRows.from_rows(q["e"])
    upd1, upd0 = e_in.empty_like(), e_in.empty_like()
    out1 = ops.edge_block(mlp, tps, tpd, q["src"], q["dst"], e_in, None, upd1, True).to_rows()
    out1n = ops.edge_block(mlp, tps, tpd, q["src"], q["dst"], e_in, None, None, True).to_rows()
    out0 = ops.edge_block(mlp, tps, tpd, q["src"], q["dst"], e_in, None, upd0, False).to_rows()
    out0n = ops.edge_block(mlp, tps, tpd, q["src"], q["dst"], e_in, None, None, False).to_rows()
    torch.cuda.synchronize()
    u1, u0 = upd1.to_rows(), upd0.to_rows()
    worst.add(ec.assert_update_matches_emulation(u1, want, f"{what}: e_upd, residual", l2_gate))
    worst.add(ec.assert_update_matches_emulation(out0, want, f"{what}: e_out, no residual", l2_gate))
    ec.assert_residual_is_f32_sum(out1, q["e"], u1, what)
    assert torch.equal(u0, out0) and torch.equal(u0, u1), f"{what}: e_upd differs between residual = 0 and 1"
    assert torch.equal(out1n, out1) and torch.equal(out0n, out0), f"{what}: e_out depends on whether e_upd is asked for"
    if alias:                                                            # e_out aliases e_in
        ops.edge_block(mlp, tps, tpd, q["src"], q["dst"], e_in, e_in, None, True)
        assert torch.equal(e_in.to_rows(), out1), f"{what}: in place"
    return mlp


def _edge_family(worst, prec, hidden, latent, counts, chained_edges):
    p_format = ops.p_table_format(prec)
    first = True
    for nh in (1, 2, 3):
        seed = 1000 * hidden + 10 * latent + nh
        packed = None
        cases = [(E, None, "random") for E in counts] + [(counts[1], 1, "random"), (counts[2], None, "last to first")]
        for E, n, graph in cases:
            p = ec.edge_problem(seed, hidden, latent, nh, E, n, graph)      # the same seed: the same weights for every E
            packed = _edge_case(worst, prec, p_format, p, f"{prec} ({hidden},{latent}) nh={nh} E={E} n={n} {graph}", packed,
                                alias=first and E == counts[2])
        first = False
    # LayerNorm input rows with |mean| of some 36 standard deviations: the output bias raised by 10
    p = ec.edge_problem(7 + hidden, hidden, latent, 2, counts[-1])
    p["lins"] = p["lins"][:-1] + [(p["lins"][-1][0], p["lins"][-1][1] + 10.0)]
    big = _Worst(f"{prec} ({hidden},{latent}) with a large LayerNorm mean")
    _edge_case(big, prec, p_format, p, big.what, l2_gate=5e-3)
    big.report()
    # chained: the tables cgnn_project_nodes writes, the emulation fed the rounded exact sums
    E, n = chained_edges, max(200, chained_edges // 8)
    p = ec.edge_problem(11 + hidden, hidden, latent, 2, E, n)
    x, ws, wd, b1 = ec.projection_problem(13 + hidden, hidden, latent, n)
    dtype = bs.P_FORMAT_DTYPE[p_format]
    p["ps"] = bs.round_to(bs.emulate_project(x, ws, None, dtype)[0].float(), dtype)
    p["pd"] = bs.round_to(bs.emulate_project(x, wd, b1, dtype)[0].float(), dtype)
    tables = ops.project_nodes(ops.PackedLinear(_dev(ws), None, "bf16"), ops.PackedLinear(_dev(wd), _dev(b1), "bf16"), _dev(x), None,
                               None, p_format)
    _edge_case(worst, prec, p_format, p, f"{prec} ({hidden},{latent}) chained to project_nodes", tables=tables)


@pytest.mark.parametrize("hidden,latent", ec.PAIRS)
def test_edge_block_bf16(hidden, latent):
    worst = _Worst(f"edge_block bf16 ({hidden},{latent})")
    _edge_family(worst, "bf16", hidden, latent, (1, 33, 4095, 4096, 4101), 4101)     # 4096: the weights move into LDS
    worst.report()


@pytest.mark.parametrize("hidden,latent", N16_PAIRS)
def test_edge_block_bf16_n16(hidden, latent):
    worst = _Worst(f"edge_block bf16_n16 ({hidden},{latent})")
    _edge_family(worst, "bf16_n16", hidden, latent, (1, 15, 16, 17, 539, 4133), 4133)
    worst.report()


def test_edge_block_ring256():
    """latent = hidden = 256 on the LDS-ring kernel: with half_tiles = 2 ceil(E / 32), E = 32 is the RAGGED launch alone,
    100 one whole step with a partial tile, 128 one whole step, 539 four steps + two half tiles, 80069 = 625 steps (more
    than a workgroup per CU) + six half tiles with a partial last tile."""
    worst = _Worst("edge_block bf16_n16 (256,256)")
    _edge_family(worst, "bf16_n16", 256, 256, (32, 100, 128, 539, 80069), 539)
    worst.report()


# ------------------------------------------------------------------ d. edge encoders
def _encoder_family(prec, hidden, latent):
    worst = _Worst(f"edge encoder {prec} ({hidden},{latent})")
    ns = (1, 15, 16, 17, 31, 32, 33, 4099)
    for nh in (1, 2, 3):
        for fin in (1, 4, 17, 32):
            p = {k: _dev(v) for k, v in ec.encoder_problem(100 * hidden + latent + 10 * nh + fin, fin, hidden, latent, nh, ns[-1]).items()}
            mlp = ops.PackedMLP(p["lins"], p["ln"], prec)
            want_all = bs.emulate_encoder(p["attr"], p["lins"], p["ln"])          # rows are independent: one emulation
            for i, n in enumerate(ns):
                x, want = p["attr"][:n].contiguous(), want_all[:n]
                what = f"{worst.what} nh={nh} in={fin} n={n}"
                got = ops.mlp_rows(mlp, x, tiled=True).to_rows()
                worst.add(ec.assert_update_matches_emulation(got, want, what + " tiled"))
                if prec != "bf16":
                    continue                                                   # CGNN_BF16_N16 writes TILED32 only
                pad = (8, 5)[i % 2]                                            # whole 16-byte stores / the ragged store path
                buf = torch.full((n + 3, latent + pad), FILL, device=DEV)
                ops.mlp_rows(mlp, x, out=buf[:n, :latent])
                torch.cuda.synchronize()
                assert torch.equal(buf[:n, :latent], got), what + ": row-major differs from tiled"
                assert bool((buf[n:] == FILL).all()) and bool((buf[:, latent:] == FILL).all()), what + ": wrote outside [n, out]"
    worst.report()


@pytest.mark.parametrize("hidden,latent", ec.PAIRS)
def test_edge_encoders_bf16(hidden, latent):
    _encoder_family("bf16", hidden, latent)


@pytest.mark.parametrize("hidden,latent", N16_PAIRS)
def test_edge_encoders_bf16_n16(hidden, latent):
    _encoder_family("bf16_n16", hidden, latent)


# ------------------------------------------------------------------ the gates, through the kernels
@pytest.mark.parametrize("prec,hidden,latent", [("bf16", 128, 128), ("bf16_n16", 128, 64), ("bf16_n16", 256, 256)])
def test_the_gates_reject_a_kernel_fed_a_slightly_wrong_model(prec, hidden, latent):
    """What test_bf16_kernel_gates_cpu.py shows with a stand-in, once with the kernels themselves: the kernel runs a model
    with one vector changed (the defects the 3e-2 norm of test_gpu_parity.py lets through), the emulation the intended
    one; and a table read in the other layout is no table."""
    p_format = ops.p_table_format(prec)
    p = {k: _dev(v) for k, v in ec.edge_problem(5, hidden, latent, 2, 539).items()}
    want = bs.emulate_edge_update(p["ps"], p["pd"], p["src"], p["dst"], p["e"], p["lins"], p["ln"])
    tps, tpd = bs.logical_to_table(p["ps"], p_format), bs.logical_to_table(p["pd"], p_format)
    e_in = ops.TiledRows.from_rows(p["e"])
    lins, (gamma, beta) = [(p["lins"][0][0], None)] + list(p["lins"][1:]), p["ln"]

    def run(lins, ln, tps=tps, tpd=tpd):
        return ops.edge_block(ops.PackedMLP(lins, ln, prec), tps, tpd, p["src"], p["dst"], e_in, None, None, False).to_rows()
    ec.assert_update_matches_emulation(run(lins, (gamma, beta)), want)
    wrong = {"bias of the hidden Linear dropped": run([lins[0], (lins[1][0], torch.zeros_like(lins[1][1])), lins[2]], (gamma, beta)),
             "beta dropped": run(lins, (gamma, torch.zeros_like(beta))),
             "gamma replaced by 1": run(lins, (torch.ones_like(gamma), beta)),
             "Pd without its bias": run(lins, (gamma, beta), tpd=bs.logical_to_table(bs.bf(p["pd_raw"]), p_format)),
             "tables in the other layout": run(lins, (gamma, beta), *(bs.logical_to_table(t, 3 - p_format) for t in (p["ps"], p["pd"])))}
    for name, got in wrong.items():
        ec.must_fail(ec.assert_update_matches_emulation, got, want, name)
    # cgnn_project_nodes: its table decoded with the other bf16 layout is rejected by the table gate
    x, ws, wd, b1 = _dev(ec.projection_problem(6, hidden, latent, 300))
    _, pd = ops.project_nodes(None, ops.PackedLinear(wd, b1, "bf16"), x, None, None, p_format)
    exact, bound = bs.emulate_project(x, wd, b1, torch.bfloat16)
    ec.assert_table_is_rounded_exact(bs.table_to_logical(pd, p_format), exact, bound, torch.bfloat16)
    ec.must_fail(ec.assert_table_is_rounded_exact, bs.table_to_logical(pd, 3 - p_format), exact, bound, torch.bfloat16)
