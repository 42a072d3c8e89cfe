"""GPU: the backward kernels (cgnn_mlp_backward, cgnn_edge_mlp_backward, cgnn_linear2_rows and the reductions behind them)
against float64 autograd, per ROW, at sizes where the persistent tile loop runs more than once per wave.

All three kernels are persistent: ``grid_for_tiles`` caps the grid at 2 workgroups of four waves per CU and ``tile_range()``
strides each wave through its XCD's eighth of the 32-row tiles, so a wave takes a second tile only above 8 CUs tiles.
``backward_checks.rows_past_one_pass()`` -- 131,239 rows on the 256 CUs of an MI355X -- is the smallest count at which
every wave runs two tiles and some a third, the eighths are uneven and the last tile is ragged (tests A, B, C); tests D
and E (389 rows) pin the overflow contract of the (fp16x2, fp32x3) pairing and the leading-dimension / alignment branches
of include/cgnn.h.  The rows of every problem are margin-filtered: a ReLU input at rounding distance from zero makes ANY
f32 gradient of its row discontinuous, so such rows are re-drawn before anything is computed (at most 2 %, asserted), and
then NOTHING is excluded from a gate.  Gates (backward_checks.py): parameters 2e-5 of each tensor's largest entry (3e-5 at
width 256), every row of every data gradient within 2e-5 of its own norm, ``dy`` rows spread over 1e-8 .. 1; torch's
float32 backward on the CPU has to meet a quarter of each gate on the same problem."""
import ctypes as C

import pytest
import torch

import backward_checks as bc
from cosmology_gnn_simulation_amd import _lib, ops, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRINGS = ["fp32", "fp32x3", "fp32x3 with the forward recomputed on fp16x2"]


def _train_mlp(p, precision):
    sd, nh = p["sd"], p["nh"]
    lins = [bc.Lin(sd[f"m.0.{2 * i}.weight"].to(DEV), sd[f"m.0.{2 * i}.bias"].to(DEV)) for i in range(nh + 1)]
    lnm = bc.Lin(sd["m.1.weight"].to(DEV), sd["m.1.bias"].to(DEV)) if p["ln"] else None
    latent_input = precision.endswith("fp16x2")
    tm = training._TrainMLP(lins, lnm, split_at=p["fin"] if p["fin2"] else None, precision=precision.split()[0],
                            latent_input=latent_input)
    assert (tm.rec.precision == _lib.F16X2) == latent_input
    return tm


def _mlp_backward(p, precision):
    """-> (du1, du2, grads) of training._TrainMLP.backward on problem ``p``."""
    tm = _train_mlp(p, precision)
    fin, fin2 = p["fin"], p["fin2"]
    scratch = ops.BackwardScratch(p["n"], p["hid"], max(p["hid"], p["out"], 32), p["nh"], DEV)
    ud = p["u"].to(DEV)
    u1 = ud[:, :fin].contiguous()
    u2 = ud[:, fin:].contiguous() if fin2 else None
    return tm.backward(u1, u2, p["dy"].to(DEV), scratch, True, True)


# ---- A -----------------------------------------------------------------------------------------------------------------
MLP_SHAPES = [(128, 128, 128, 128, 2, True),      # node model
              (17, 0, 128, 128, 2, True),         # encoder, ragged input
              (128, 0, 128, 3, 2, False),         # decoder, ragged output, no LayerNorm
              (256, 256, 256, 256, 1, True),      # latent 256
              (64, 64, 128, 64, 3, True)]         # hidden differs from latent


@pytest.mark.parametrize("precision", PAIRINGS)          # (the pairings of one shape run back to back and share its oracle)
@pytest.mark.parametrize("fin,fin2,hid,out,nh,ln", MLP_SHAPES)
def test_mlp_backward_per_row_past_one_tile_per_wave(fin, fin2, hid, out, nh, ln, precision):
    """cgnn_mlp_backward + the parameter-gradient reductions (training._TrainMLP.backward) at rows_past_one_pass() rows --
    every wave of the tile loop runs two tiles, some three; uneven XCD eighths; ragged last tile; scratch rows written by
    a wave's second tile -- against float64 autograd: du1 / du2 per row, parameters per tensor.  Rows are margin-filtered
    (see the module docstring), dy rows span 1e-8 .. 1."""
    n = bc.rows_past_one_pass()
    p, want, yard = bc.mlp_case(fin + fin2 + hid + out + nh, n, fin, fin2, hid, out, nh, ln)
    du1, du2, grads = _mlp_backward(p, precision)
    st = bc.check_mlp(p, want, du1, du2, grads, f"mlp {(fin, fin2, hid, out, nh, ln)} {precision}")
    bc.report(f"mlp_backward {(fin, fin2, hid, out, nh, ln)} n={n} [{precision}]", st, yard)


# ---- B -----------------------------------------------------------------------------------------------------------------
def _edge_backward(p, precision):
    """One round's edge backward as training._EdgeStreams runs it: ops.edge_mlp_backward, training.edge_round_grads,
    ops.linear2_rows.  -> dict(de, dx, dps, dpd, dy, grads, inplace): ``inplace`` the de of the in-place / row-major run."""
    sd, nh, D, H, n, ne = p["sd"], p["nh"], p["D"], p["H"], p["n"], p["ne"]
    lins = [bc.Lin(sd[f"m.0.{2 * i}.weight"].to(DEV), sd[f"m.0.{2 * i}.bias"].to(DEV)) for i in range(nh + 1)]
    lnm = bc.Lin(sd["m.1.weight"].to(DEV), sd["m.1.bias"].to(DEV))
    prec = precision.split()[0]
    te = training._TrainEdge(lins, lnm, D, prec)
    if prec == "fp32x3":      # the (fp32x3, fp32x3) or the (fp16x2, fp32x3) pairing at every shape
        rec = "fp16x2" if precision.endswith("fp16x2") else "fp32x3"
        te.rec = ops.PackedMLP([(l.weight, l.bias) for l in lins], (lnm.weight, lnm.bias), rec, first_layer_cols=(2 * D, D))
    assert (te.rec.precision == _lib.F16X2) == precision.endswith("fp16x2")
    xd, srcd, dstd = p["x"].to(DEV), p["src"].to(DEV), p["dst"].to(DEV)
    ps, pd = ops.project_nodes(te.ws, te.wd, xd, p_format=_lib.P_F32)
    et = ops.TiledRows.from_rows(p["e"].to(DEV))
    de = ops.TiledRows.from_rows(p["de_next"].to(DEV))
    d_agg = p["d_agg"].to(DEV)
    scratch = ops.BackwardScratch(ne, H, D, nh, DEV)
    dy = torch.empty(ne, D, device=DEV)
    by_sender = ops.SenderCsr(srcd, None, n)
    by_receiver = ops.SenderCsr(dstd, None, n) if p["fixed_k"] == 0 else None
    de_sep = de.empty_like()
    ops.edge_mlp_backward(te.rec, te.bwd, ps, pd, srcd, dstd, et, d_agg, de, scratch, dy, de_sep)
    dy_first = dy.clone()
    grads, dps, dpd = training.edge_round_grads(te, scratch, dy, et, xd, dstd, p["fixed_k"], by_sender, by_receiver)
    dx = ops.linear2_rows(te.wst, te.wdt, dps, dpd)
    # in place (de_out = de_in), and d e written in rows (what the edge encoder's backward reads)
    ops.edge_mlp_backward(te.rec, te.bwd, ps, pd, srcd, dstd, et, d_agg, de, scratch, dy, de.buf, de_out_rows=True)
    return dict(de=de_sep.to_rows(), dx=dx, dps=dps, dpd=dpd, dy=dy_first, grads=grads, inplace=de.buf[:ne])


def _edge_nodes(graph, ne):
    """Nodes for at most ``ne`` edges: E rounded down to a multiple of k (fixed k), or to 5 n + 3 (general list)."""
    return (ne - 3) // 5 if graph == "general" else ne // int(graph[1:])


@pytest.mark.parametrize("precision", PAIRINGS)
@pytest.mark.parametrize("H,D,nh,graph", [(128, 128, 2, "k16"), (256, 256, 1, "general"), (128, 64, 3, "k8")])
def test_edge_backward_per_row_past_one_tile_per_wave(H, D, nh, graph, precision):
    """cgnn_edge_mlp_backward, training.edge_round_grads and linear2_rows with rows_past_one_pass() edges (rounded down to
    the graph's shape; still two to three tiles per wave, asserted): de, dPs, dPd and dx per row and every parameter per
    tensor against float64 autograd of L = <e + u, de_next> + <agg(u), d_agg>; dy = de_next + d_agg[dst] within 1e-6;
    the in-place, row-major run bit-identical.  Rows of de_next and d_agg span 1e-8 .. 1; edges are margin-filtered."""
    n = _edge_nodes(graph, bc.rows_past_one_pass())
    p, want, yard = bc.edge_case(1000 + H + D + nh, H, D, nh, graph, n)
    bc.assert_runs_passes(p["ne"])
    got = _edge_backward(p, precision)
    assert bc.close(got["dy"], want["dy"], 1e-6)
    st = bc.check_edge(p, want, got, f"edge {(H, D, nh, graph)} {precision}")
    assert torch.equal(got["inplace"], got["de"])
    bc.report(f"edge_mlp_backward {(H, D, nh, graph)} E={p['ne']} [{precision}]", st, yard)


# ---- C -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("addends", [0, 1, 2])
@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
@pytest.mark.parametrize("width", [128, 256])
def test_linear2_rows_per_row_past_one_tile_per_wave(width, precision, addends):
    """cgnn_linear2_rows on its own at rows_past_one_pass() rows (inside a training step it runs over the nodes: 29-37
    rows in the other tests): out = [add1 +] [add2 +] a Wa^T + b Wb^T per row against float64, rows x 1e-8 .. 1; with two
    addends ``out`` is ``add1`` itself."""
    n = bc.rows_past_one_pass()
    p, want = bc.linear2_case(width, n, width, width)
    wa, wb = ops.PackedLinear(p["wa"].to(DEV), None, precision), ops.PackedLinear(p["wb"].to(DEV), None, precision)
    a, b = p["a"].to(DEV), p["b"].to(DEV)
    add1, add2 = p["add1"].to(DEV), p["add2"].to(DEV)
    if addends == 0:
        out = ops.linear2_rows(wa, wb, a, b)
    elif addends == 1:
        out = ops.linear2_rows(wa, wb, a, b, add1=add1)
        assert torch.equal(add1.cpu(), p["add1"])
    else:
        out = ops.linear2_rows(wa, wb, a, b, add1=add1, add2=add2, out=add1)
        assert out is add1
    worst = bc.assert_rows(out, want[addends], f"linear2_rows {width} {precision} addends={addends}")
    print(f"backward-gate linear2_rows {width}->{width} n={n} [{precision}] addends={addends}: worst-row {worst:.2e} "
          f"max-norm {bc.max_norm_err(out, want[addends]):.2e}")


# ---- D -----------------------------------------------------------------------------------------------------------------
SPIKE_ROW, SPIKE_COL, SPIKE = 137, 5, 7e4        # 7e4 > 65504: no fp16 value


def _assert_loud(p, grads, clean):
    """Every parameter gradient of a call with an overflowed row holds no finite value (each is a sum over all rows of
    products with that row's NaN) -- but LayerNorm's dbeta, the column sums of dy, which no forward value enters."""
    for name, g, c in zip(bc.param_names(p["nh"]), grads, clean, strict=True):
        if name == "m.1.bias":
            assert torch.equal(g, c), name
        else:
            assert not bool(torch.isfinite(g).any()), f"{name}: finite values although row {SPIKE_ROW} overflowed"


@pytest.mark.parametrize("precision", PAIRINGS)
def test_mlp_backward_range_contract(precision):
    """One input value of 7e4 in row 137 of 389.  Under (fp16x2, fp32x3) the recomputed forward overflows fp16 and the
    kernel's contract is "NaN stays NaN (an fp16 overflow must show)": every du value of that row is non-finite, every other
    row has the bits of the clean run, and every parameter gradient of the call that a forward value enters is non-finite
    (all but LayerNorm's dbeta = colsum(dy)) -- the loud part.  Under
    fp32 and fp32x3 (f32 exponent range) the same input stays finite and meets the gates."""
    n = 389
    p, want, yard = bc.mlp_case(101, n, 128, 128, 128, 128, 2, True)
    q = bc.with_spike(p, "u", SPIKE_ROW, SPIKE_COL, SPIKE)
    du1, du2, grads = _mlp_backward(q, precision)
    if not precision.endswith("fp16x2"):
        wq, yq = bc.mlp_case_of(q)
        bc.report(f"mlp_backward with 7e4 in one row [{precision}]", bc.check_mlp(q, wq, du1, du2, grads, precision), yq)
        return
    c1, c2, cgrads = _mlp_backward(p, precision)
    bc.check_mlp(p, want, c1, c2, cgrads, "clean run")
    others = torch.arange(n, device=DEV) != SPIKE_ROW
    for got, clean, name in ((du1, c1, "du1"), (du2, c2, "du2")):
        assert not bool(torch.isfinite(got[SPIKE_ROW]).any()), f"{name}: row {SPIKE_ROW} holds finite values after an fp16 overflow"
        assert torch.equal(got[others], clean[others]), name
    _assert_loud(p, grads, cgrads)


@pytest.mark.parametrize("precision", PAIRINGS)
def test_edge_backward_range_contract(precision):
    """The same contract for cgnn_edge_mlp_backward: 7e4 in one value of edge 137's latent (389 edges on 50 nodes)."""
    p, want, yard = bc.edge_case(201, 128, 128, 2, "general", 50, 389)
    q = bc.with_spike(p, "e", SPIKE_ROW, SPIKE_COL, SPIKE)
    got = _edge_backward(q, precision)
    if not precision.endswith("fp16x2"):
        wq, yq = bc.edge_case_of(q)
        bc.report(f"edge_mlp_backward with 7e4 in one row [{precision}]", bc.check_edge(q, wq, got, precision), yq)
        return
    clean = _edge_backward(p, precision)
    bc.check_edge(p, want, clean, "clean run")
    others = torch.arange(p["ne"], device=DEV) != SPIKE_ROW
    assert not bool(torch.isfinite(got["de"][SPIKE_ROW]).any()), f"de: row {SPIKE_ROW} holds finite values after an fp16 overflow"
    assert torch.equal(got["de"][others], clean["de"][others]) and torch.equal(got["dy"], clean["dy"])
    assert torch.equal(got["inplace"][others], clean["de"][others]) and not bool(torch.isfinite(got["inplace"][SPIKE_ROW]).any())
    hit = torch.zeros(p["n"], dtype=torch.bool, device=DEV)                  # the two nodes of that edge
    hit[int(p["src"][SPIKE_ROW])] = hit[int(p["dst"][SPIKE_ROW])] = True
    for k in ("dps", "dpd", "dx"):
        assert torch.equal(got[k][~hit], clean[k][~hit]), k
    _assert_loud(p, got["grads"], clean["grads"])


# ---- E -----------------------------------------------------------------------------------------------------------------
SENTINEL = -777.0


def _strided(t, ld, offset, fill, extra_rows=3):
    """-> (flat buffer, an [n, w] view of it with row stride ``ld`` starting ``offset`` floats past the allocation's
    16-byte-aligned start, holding ``t``); everything else in the buffer holds ``fill``."""
    n, w = t.shape
    flat = torch.full((offset + (n + extra_rows) * ld + 8,), fill, dtype=torch.float32, device=DEV)
    view = flat[offset:].as_strided((n, w), (ld, 1))
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.data_ptr() == flat.data_ptr() + 4 * offset
    return flat, view


def _untouched_outside(flat, view, fill):
    """Everything of ``flat`` outside ``view`` still holds ``fill`` (``view`` is overwritten by this check)."""
    view.fill_(fill)
    return bool((flat == fill).all())


def _raw_mlp_backward(tm, u1, u2, dy, n, scratch, du1, du2):
    bufs = scratch.struct(tm.nh, tm.out_padded)
    s_f2 = tm.rec2.struct() if tm.rec2 is not None else None
    s_b2 = tm.bwd2.struct() if tm.bwd2 is not None else None
    ops.check(_lib.load().cgnn_mlp_backward(
        C.byref(tm.rec.struct()), C.byref(s_f2) if s_f2 is not None else None, C.byref(tm.bwd.struct()),
        C.byref(s_b2) if s_b2 is not None else None, u1.data_ptr(), u1.stride(0), ops.ptr(u2),
        u2.stride(0) if u2 is not None else 0, dy.data_ptr(), dy.stride(0), n, C.byref(bufs), du1.data_ptr(), du1.stride(0),
        ops.ptr(du2), du2.stride(0) if du2 is not None else 0, ops.stream_ptr(u1.device)), "cgnn_mlp_backward")


def _scratch_rows(scratch, tm, n):
    return [t[:n].clone() for t in scratch.h[:tm.nh] + scratch.g_a[:tm.nh]] + \
        [scratch.g_o.view(-1)[:n * tm.out_padded].clone()] + \
        ([scratch.zhat.view(-1)[:n * tm.out_padded].clone()] if tm.ln is not None else [])


LAYOUTS = [dict(ld1=2), dict(ld_dy=4), dict(ld_du1=1), dict(off_u1=1, off_dy=1), dict(ld1=2, ld_dy=4, ld_du1=1, off_u1=1, off_dy=1),
           dict(ld1=4, ld_du1=4), dict(off_u1=1), dict(off_dy=1)]


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
@pytest.mark.parametrize("fin,fin2,hid,out,nh,ln", [(128, 128, 128, 128, 2, True), (17, 0, 128, 128, 2, True),
                                                    (128, 0, 128, 3, 2, False)])
def test_mlp_backward_leading_dimensions_and_alignment(fin, fin2, hid, out, nh, ln, precision):
    """cgnn_mlp_backward through the C ABI with the layouts include/cgnn.h allows besides contiguous, 16-byte-aligned
    matrices: ld1 = in1 + 2 (in1_full off: load_rows_ragged / store_rows_ragged at full width), ld_dy = out + 4 (the
    16-byte path with a row stride), ld_du1 = in1 + 1 (ragged stores), u1 and dy starting 4 bytes past a 16-byte boundary
    (ragged loads of both), all of these at once, and padded leading dimensions that keep the 16-byte paths.  du1, du2 and
    every scratch matrix equal the contiguous call bit for bit (same sums, same order); the padding columns of u1 / dy
    hold NaN and are never read; sentinel-filled padding columns and trailing rows of du1 stay untouched.  The ragged
    shapes are the encoder (17 inputs: never 16-byte rows) and the decoder (3 outputs, no LayerNorm); an MLP ragged at
    both ends (17 -> 128 -> 3) is no model of the project and has no kernel: test_mlp_backward_refuses_an_mlp_ragged_at_both_ends."""
    n = 389
    p = bc.mlp_problem(fin + out, n, fin, fin2, hid, out, nh, ln)
    tm = _train_mlp(p, precision)
    ud = p["u"].to(DEV)
    u1 = ud[:, :fin].contiguous()
    u2 = ud[:, fin:].contiguous() if fin2 else None
    dy = p["dy"].to(DEV)
    scratch = ops.BackwardScratch(n, hid, tm.out_padded, nh, DEV)
    du1 = torch.full((n, fin), SENTINEL, device=DEV)
    du2 = torch.full((n, fin2), SENTINEL, device=DEV) if fin2 else None
    _raw_mlp_backward(tm, u1, u2, dy, n, scratch, du1, du2)
    base = [du1.clone()] + ([du2.clone()] if fin2 else []) + _scratch_rows(scratch, tm, n)
    assert all(bool(torch.isfinite(t).all()) for t in base) and not bool((du1 == SENTINEL).any())
    want = bc.mlp_reference(p)                                              # and the contiguous call is right
    assert bc.assert_rows(du1, want["du"][:, :fin], "du1") <= bc.GTOL
    for lay in LAYOUTS:
        nan = float("nan")
        _, u1v = _strided(u1, fin + lay.get("ld1", 0), lay.get("off_u1", 0), nan)
        _, dyv = _strided(dy, out + lay.get("ld_dy", 0), lay.get("off_dy", 0), nan)
        flat_du1, du1v = _strided(torch.full((n, fin), SENTINEL, device=DEV), fin + lay.get("ld_du1", 0), 0, SENTINEL)
        for t in scratch.h + scratch.g_a + [scratch.g_o, scratch.zhat]:
            t.fill_(SENTINEL)
        if du2 is not None:
            du2.fill_(SENTINEL)
        _raw_mlp_backward(tm, u1v, u2, dyv, n, scratch, du1v, du2)
        got = [du1v.clone()] + ([du2.clone()] if fin2 else []) + _scratch_rows(scratch, tm, n)
        for i, (g, b) in enumerate(zip(got, base, strict=True)):
            assert torch.equal(g, b), f"{lay}: result {i} differs from the contiguous call"
        assert _untouched_outside(flat_du1, du1v, SENTINEL), f"{lay}: du1's padding was written"


def test_mlp_backward_refuses_an_mlp_ragged_at_both_ends():
    """(17, 0, 128, 3, 2, False): cgnn_mlp_backward is compiled for encoders (narrow input, latent output) and decoders
    (latent input, narrow output), not for both at once -- refused before launch, nothing written."""
    p = bc.mlp_problem(20, 389, 17, 0, 128, 3, 2, False)
    tm = _train_mlp(p, "fp32")
    scratch = ops.BackwardScratch(389, 128, 32, 2, DEV)
    du1 = torch.full((389, 17), SENTINEL, device=DEV)
    with pytest.raises(ops.CgnnError, match="no kernel for in=\\(17,0\\) hidden=128 out=3"):
        _raw_mlp_backward(tm, p["u"].to(DEV), None, p["dy"].to(DEV), 389, scratch, du1, None)
    torch.cuda.synchronize()
    assert bool((du1 == SENTINEL).all())
