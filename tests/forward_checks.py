"""Problems, gates and guards for the forward kernels that claim f32 accuracy (CGNN_F32, CGNN_F32X3, CGNN_F16X2, CGNN_F32X3_N16,
CGNN_F16X2_N16 through cgnn_mlp_rows, cgnn_project_nodes, cgnn_node_block and cgnn_edge_block): they can see ONE wrong row among
10^5, at sizes where a wave of a persistent tile loop takes a second tile, and a write or a read outside the arguments (test
infrastructure, in the style of backward_checks.py; imports no engine code: the CPU file tests it without a GPU).

* geometry: ``grid_for_tiles`` / ``tile_range`` are backward_checks's restatement (csrc/runtime.hip, csrc/cgnn_common.hpp);
  ``LAUNCHES`` restates each launcher's (rows per tile, workgroups per CU, waves per workgroup); ``rows_past_one_pass`` is the
  smallest row count at which every wave (every workgroup of the block-uniform kernels) runs ``passes`` tiles and some one more,
  with uneven XCD eighths and a ragged last tile; ``ring_steps`` / ``ring_rows_past_one_pass`` are the twin for the step loops
  of node_block_f2.hip / edge_block_f2.hip (``grid = min(steps, CUs)``, stride ``grid``, 128 rows per step).
* problems: a row MLP, a node update, an edge update and a projection, seeded, with the row scales of
  edge_checks.projection_problem (3 randn, one block of 50 rows x 1e-3, one x 30: inside the two-fp16-term range); the float64
  reference and the float32 yardstick (the same operation in torch float32 on the CPU) are cached per shape.
* gates: the tensor contract ``max |err| <= 2e-6 max |want|`` and, for EVERY row, ``||got_row - want_row|| <= G ||want_row||``
  with G = 4 x the yardstick's worst row on the same problem (the matrix cores sum in another order than a BLAS and the split
  formats drop terms of <= 2^-22: the margin of the reduction gates), G <= 1e-5 asserted (the model-level f32 gate).
* guards: inputs are row slices of NaN-filled buffers (NaN columns where the entry takes a leading dimension), outputs are
  views into canary-filled buffers; every canary byte must survive, and a NaN in a result is a read outside an input.
"""
import functools

import torch
import torch.nn.functional as F

import backward_checks as bc
import edge_checks as ec
from backward_checks import device_cus, grid_for_tiles, tile_range  # noqa: F401  (one restatement for both files)

TENSOR_TOL = 2e-6           # the project's f32 contract: max |err| <= 2e-6 max |want| over the tensor
G_CAP = 1e-5                # the model-level f32 gate (tests/test_gpu_fullsize.py): no per-row gate may be looser
G_FACTOR = 4.0
RING_ROWS = 128             # rows per step of the two-waves-per-SIMD ring kernels

# ---- geometry ---------------------------------------------------------------------------------------------------------------
# launch -> (rows per tile, workgroups per CU, waves per workgroup), restated from the launchers:
LAUNCHES = {
    "rows32": (32, 2, 4),        # mlp_rows_kernel / project_kernel / node_block_kernel / edge_block_kernel<CGNN_F32>, weights from L2
    "rows32_lds": (32, 1, 4),    # mlp_rows_kernel<.., WLDS = true> (launch_mlp_rows: WLDS ? 1 : 2)
    "node_x3": (32, 1, 4),       # node_block_x3_kernel (launch_node_x3: grid_for_tiles(tiles, 1)), block-uniform loop
    "node_n16": (16, 1, 8),      # node_block_x3n16_kernel / node_block_f2n16_kernel: CGNN_NODE_N16_BPC, CGNN_NODE_N16_BLOCK / 64
}
LDS_ROWS = 4096                  # cgnn_mlp_rows / cgnn_project_nodes keep two-fp16-term weights in LDS from this many rows on
X3_ROWS = 2048                   # cgnn_node_block takes node_block_x3_kernel from this many rows on


def project_launch(precision, latent, hidden, n):
    """cgnn_project_nodes -> CGNN_P_F32 (launch_project): LDS weights for two fp16 terms (4 bytes per weight) when both
    matrices fit 152 KiB and n >= 4096; then one workgroup per CU if ``2 * wbytes > 76 KiB`` else two."""
    wbytes = latent * hidden * 4
    if precision == "fp16x2" and 2 * wbytes <= 152 * 1024 and n >= LDS_ROWS:
        return "rows32_lds" if 2 * wbytes > 76 * 1024 else "rows32"
    return "rows32"


def wave_tile_counts(n, launch, cus):
    """-> (tiles, the number of tiles every wave of the launch for ``n`` rows runs, in workgroup-major order).  For the
    block-uniform kernels a workgroup's trip count is the largest count among its waves."""
    rows, bpc, waves = LAUNCHES[launch]
    tiles = (n + rows - 1) // rows
    nb = grid_for_tiles(tiles, cus, bpc, waves)
    return tiles, [len(tile_range(tiles, nb, b, w, waves)) for b in range(nb) for w in range(waves)]


def assert_runs_passes(n, launch, passes=2, cus=None):
    """Every wave runs at least ``passes`` tiles, some run one more, the XCD eighths are uneven, the last tile is ragged."""
    cus = device_cus() if cus is None else cus
    rows, bpc, waves = LAUNCHES[launch]
    tiles, counts = wave_tile_counts(n, launch, cus)
    nb = grid_for_tiles(tiles, cus, bpc, waves)
    assert nb % 8 == 0 and min(counts) >= passes and max(counts) > min(counts), (n, launch, cus, min(counts), max(counts))
    assert tiles % 8 != 0 and n % rows != 0, (n, launch, tiles)
    return n


def rows_past_one_pass(rows_per_tile, blocks_per_cu, waves, passes=2, cus=None):
    """The smallest row count of this shape (five tiles and seven rows past ``passes`` sweeps of the full grid) at which every
    wave runs ``passes`` tiles and some one more; the properties are asserted, not assumed."""
    cus = device_cus() if cus is None else cus
    launch = next(k for k, v in LAUNCHES.items() if v == (rows_per_tile, blocks_per_cu, waves))
    nb = grid_for_tiles(1 << 40, cus, blocks_per_cu, waves)
    return assert_runs_passes(rows_per_tile * (waves * nb * passes + 5) + 7, launch, passes, cus)


def past_one_pass(launch, passes=2, cus=None):
    return rows_past_one_pass(*LAUNCHES[launch], passes=passes, cus=cus)


def ring_steps(n, cus):
    """node_block_f2.hip: steps of 128 rows, ``grid = min(steps, CUs)``, workgroup b runs steps b, b + grid, ...
    -> (steps, grid, [steps per workgroup])."""
    steps = (n + RING_ROWS - 1) // RING_ROWS
    grid = min(steps, cus)
    return steps, grid, [len(range(b, steps, grid)) for b in range(grid)]


def edge_ring_steps(ne, cus):
    """edge_block_f2.hip: the TILED32 buffers hold whole 32-row tiles = 2 half tiles of 16; the full launch runs
    ``half_tiles // 8`` steps like the node ring, a second (RAGGED) launch of one step the remaining half tiles.
    -> (full steps, grid, [steps per workgroup], half tiles of the ragged launch)."""
    half_tiles = 2 * ((ne + 31) // 32)
    full = half_tiles // 8
    grid = min(full, cus)
    return full, grid, [len(range(b, full, grid)) for b in range(grid)], half_tiles % 8


def ring_rows_past_one_pass(passes=2, cus=None, edge=False):
    """Every workgroup of the step loop runs ``passes`` steps, six run one more (five for the edge kernel's full-step launch), and the
    last step is partial (7 rows; for the edge kernel: one 32-row tile, the RAGGED launch)."""
    cus = device_cus() if cus is None else cus
    n = RING_ROWS * (cus * passes + 5) + 7
    if edge:
        full, grid, per, ragged = edge_ring_steps(n, cus)
        assert grid == cus and min(per) == passes and max(per) == passes + 1 and ragged == 2, (n, cus, full, ragged)
    else:
        steps, grid, per = ring_steps(n, cus)
        assert grid == cus and min(per) == passes and max(per) == passes + 1 and n % RING_ROWS != 0, (n, cus, steps)
    return n


def second_pass_row(n, launch, cus):
    """A row of the tile that wave 0 of workgroup 0 reaches in its SECOND trip, and that tile's distance from its first."""
    rows, bpc, waves = LAUNCHES[launch]
    tiles = (n + rows - 1) // rows
    tr = tile_range(tiles, grid_for_tiles(tiles, cus, bpc, waves), 0, 0, waves)
    assert len(tr) >= 2
    return tr[1] * rows + 3, (tr[1] - tr[0]) * rows


# ---- problems ---------------------------------------------------------------------------------------------------------------
def _layers(gen, dims, fan_in0=None):
    return [ec.rand_linear(gen, dims[i + 1], dims[i], fan_in0 if i == 0 else None) for i in range(len(dims) - 1)]


def mlp_problem(seed, n, fin, hid, out, nh, ln):
    """y = [LayerNorm](MLP(x)): an encoder (narrow input, LayerNorm) or a decoder (narrow output, none)."""
    gen = torch.Generator().manual_seed(seed)
    lins = _layers(gen, [fin] + [hid] * nh + [out])
    lnp = ec.rand_layer_norm(gen, out) if ln else None
    p = dict(kind="mlp", lins=lins, ln=lnp, x=ec.node_rows(gen, n, fin), n=n, nh=nh, redrawn=0)
    if not ln:
        p["redrawn"] = _redraw_cancelling_rows(gen, p)
    return p


CANCEL = 3 * 2.0 ** -24 / (0.25 * G_CAP)       # 0.0715: ||y_row|| / ||(|h| |W|^T + |b|)_row|| below which a decoder row is re-drawn
REDRAW_CAP = 0.08           # 5.5 % of the rows of a 128 -> 128 -> 3 decoder fall below CANCEL


def cancelling_rows(p, rows=slice(None)):
    """Rows of an MLP WITHOUT LayerNorm whose few outputs cancel: ||y|| < CANCEL x ||mag||, mag = |h| |W|^T + |b| the sum of the
    magnitudes of the output layer's terms (float64).  Every f32 evaluation rounds relative to its partial sums, which are of
    the size of mag, not of y: ONE rounding of 2^-24 mag is 2.5e-6 of y -- the whole quarter of the cap the yardstick has to
    meet -- at ||y|| = 0.024 ||mag||; CANCEL leaves room for three (with two, the yardstick's worst of 131,239 rows measured 2.59e-6).
    With three outputs of a 128-term sum the typical ratio is 0.14, and among 131,239 rows the smallest is near 0.003: rows on
    which NO f32 evaluation meets 1e-5 of the row's norm."""
    h = p["x"][rows].double()
    for w, b in p["lins"][:-1]:
        h = torch.relu(h @ w.double().t() + b.double())
    w, b = p["lins"][-1]
    y = h @ w.double().t() + b.double()
    mag = h.abs() @ w.double().abs().t() + b.double().abs()
    return y.norm(dim=1) < CANCEL * mag.norm(dim=1)


def _redraw_cancelling_rows(gen, p):
    """Re-draw (from ``gen``, at the row's own scale) every row :func:`cancelling_rows` names until none is left, as
    backward_checks re-draws its fragile rows; at most 8 % of the rows (asserted), nothing is excluded from a gate afterwards."""
    n, d = p["x"].shape
    scale = 3 * torch.ones(n)
    if n >= 200:
        scale[60:110] *= 1e-3
        scale[130:180] *= 30
    idx, total = torch.arange(n), 0
    for _ in range(64):
        idx = idx[cancelling_rows(p, idx)]
        if idx.numel() == 0:
            break
        total += idx.numel()
        p["x"][idx] = torch.randn(idx.numel(), d, generator=gen) * scale[idx, None]
    else:
        raise AssertionError("cancelling rows remain after 64 re-draws")
    assert total <= REDRAW_CAP * max(n, 200), f"{total} of {n} rows re-drawn (cap {REDRAW_CAP:.0%})"
    return total


def node_problem(seed, n, D, H, nh):
    """u = LayerNorm(MLP(cat[x, agg])), x_out = x + u."""
    gen = torch.Generator().manual_seed(seed)
    lins = _layers(gen, [2 * D] + [H] * nh + [D])
    lnp = ec.rand_layer_norm(gen, D)
    return dict(kind="node", lins=lins, ln=lnp, x=ec.node_rows(gen, n, D), agg=ec.node_rows(gen, n, D), n=n, nh=nh, D=D, H=H)


def edges(gen, n, ne, graph):
    """"general": unsorted random src / dst; "k<K>": receiver-sorted, K edges per receiver (ne = n K).  Both span 0 .. n - 1."""
    if graph == "general":
        src = torch.randint(0, n, (ne,), generator=gen, dtype=torch.int32)
        dst = torch.randint(0, n, (ne,), generator=gen, dtype=torch.int32)
    else:
        k = int(graph[1:])
        assert ne == n * k, (n, ne, graph)
        src = torch.randint(0, n, (ne,), generator=gen, dtype=torch.int32)
        dst = torch.arange(n, dtype=torch.int32).repeat_interleave(k)
        src[0], src[-1] = 0, n - 1
        return src, dst
    src[0], dst[0], src[-1], dst[-1] = 0, n - 1, n - 1, 0
    return src, dst


def edge_problem(seed, ne, n, D, H, nh, graph="general"):
    """u = LayerNorm(MLP(ps[src] + pd[dst] + We e)), e_out = e + u, on given f32 tables (the first layer's bias lives in pd)."""
    gen = torch.Generator().manual_seed(seed)
    lins = _layers(gen, [D] + [H] * nh + [D], 3 * D)
    lins[0] = (lins[0][0], None)
    lnp = ec.rand_layer_norm(gen, D)
    ps, pd = ec.node_rows(gen, n, H) / 3, ec.node_rows(gen, n, H) / 3 + ec.rand_linear(gen, H, 1, 3 * D)[1]
    src, dst = edges(gen, n, ne, graph)
    return dict(kind="edge", lins=lins, ln=lnp, ps=ps, pd=pd, src=src, dst=dst, e=ec.node_rows(gen, ne, D), n=ne, nodes=n, nh=nh,
                D=D, H=H)


def projection_problem(seed, n, D, H):
    x, ws, wd, b1 = ec.projection_problem(seed, H, D, n)
    return dict(kind="proj", x=x, ws=ws, wd=wd, b1=b1, n=n, D=D, H=H)


# ---- the operation, in any dtype, with the defects the CPU test plants ----------------------------------------------------------
DEFECTS = ("output bias dropped", "beta dropped", "residual missing", "one fp16 term")


def _first_layer(p, dtype, rows):
    t = lambda v: v.to(dtype)   # noqa: E731
    w0, b0 = p["lins"][0]
    if p["kind"] == "mlp":
        return t(p["x"][rows]) @ t(w0).t() + t(b0)
    if p["kind"] == "node":
        return torch.cat([t(p["x"][rows]), t(p["agg"][rows])], dim=1) @ t(w0).t() + t(b0)
    src, dst = p["src"][rows].long(), p["dst"][rows].long()
    return t(p["ps"])[src] + t(p["pd"])[dst] + t(p["e"][rows]) @ t(w0).t()


def forward(p, dtype=torch.float64, rows=slice(None), defect=None):
    """-> dict of the problem's outputs in ``dtype``: mlp ``y``; node ``u``, ``x_out``; edge ``u``, ``e_out``; projection
    ``ps``, ``pd``.  ``defect`` (one of DEFECTS) evaluates a wrong kernel."""
    assert defect is None or defect in DEFECTS
    t = lambda v: v.to(dtype)   # noqa: E731
    if p["kind"] == "proj":
        x = t(p["x"][rows])
        return dict(ps=x @ t(p["ws"]).t(), pd=x @ t(p["wd"]).t() + t(p["b1"]))
    one_term = (lambda v: v.half().to(dtype)) if defect == "one fp16 term" else (lambda v: v)
    h = _first_layer(p, dtype, rows)
    for i in range(1, p["nh"] + 1):
        w, b = p["lins"][i]
        h = one_term(torch.relu(h)) @ t(w).t()
        if not (i == p["nh"] and defect == "output bias dropped"):
            h = h + t(b)
    if p["ln"] is not None:
        g, beta = p["ln"]
        h = F.layer_norm(h, (h.shape[1],), t(g), None if defect == "beta dropped" else t(beta), 1e-5)
    if p["kind"] == "mlp":
        return dict(y=h)
    base = t((p["x"] if p["kind"] == "node" else p["e"])[rows])
    out = h if defect == "residual missing" else base + h
    return dict(u=h, x_out=out) if p["kind"] == "node" else dict(u=h, e_out=out)


# ---- gates ------------------------------------------------------------------------------------------------------------------
def tensor_err(got, want):
    return bc.max_norm_err(got, want)


def row_err(got, want):
    return ec.row_rel_max(got.detach().cpu().double(), want.detach().double())


def gate_from_yardstick(yard_worst_row, what):
    """G = 4 x the float32 yardstick's worst row, refused above the model-level gate: a problem whose own f32 evaluation is
    that bad would loosen the gate -- change the problem."""
    G = G_FACTOR * yard_worst_row
    assert 0.0 < G <= G_CAP, f"{what}: the float32 yardstick's worst row {yard_worst_row:.3e} x {G_FACTOR:g} leaves the cap {G_CAP:.0e}"
    return G


def assert_rows(got, want, G, what):
    """The tensor contract and EVERY row within G of its own norm (a NaN anywhere fails both).  -> (tensor err, worst row)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values (a read outside the inputs shows up as NaN)"
    terr = tensor_err(got, want)
    assert terr <= TENSOR_TOL, f"{what}: max |err| / max |want| = {terr:.3e} (contract {TENSOR_TOL:.0e})"
    worst, where = row_err(got, want)
    assert worst <= G, f"{what}: row {where} differs by {worst:.3e} of its norm (gate G = {G:.3e})"
    return terr, worst


def check(case, got, what, names=None):
    """Every output of ``got`` (dict name -> tensor) against the case's reference at the case's gates; prints one line per
    output (``pytest -s``: DESIGN.md section 7b).  -> {name: worst row}."""
    _, want, yard, G = case
    out = {}
    for name in names or got:
        n = got[name].shape[0]          # a kernel may have been given the first n rows of the problem (rows are independent)
        terr, worst = assert_rows(got[name], want[name][:n], G[name], f"{what} {name}")
        print(f"forward-gate {what} {name}: n={n} max-norm {terr:.2e} worst-row {worst:.2e} | G {G[name]:.2e} "
              f"yardstick worst-row {yard[name]:.2e}")
        out[name] = worst
    return out


def assert_residual_sum(e_out, e_in, e_upd, what):
    """e_out element-wise within 2^-22 max(|e_in|, |u|) of e_in + e_upd (two f32 roundings), as the bf16 gates do."""
    ec.assert_residual_is_f32_sum(e_out.cpu(), e_in.cpu(), e_upd.cpu(), what)


def case_of(p):
    """-> (problem, float64 reference, {name: the yardstick's worst row}, {name: G}); treat as read-only."""
    want = forward(p)
    yard32 = forward(p, torch.float32)
    yard = {k: row_err(yard32[k], want[k])[0] for k in want}
    G = {k: gate_from_yardstick(yard[k], f"{p['kind']} {k}") for k in want}
    return p, want, yard, G


@functools.lru_cache(maxsize=3)
def mlp_case(seed, n, fin, hid, out, nh, ln):
    return case_of(mlp_problem(seed, n, fin, hid, out, nh, ln))


@functools.lru_cache(maxsize=3)
def node_case(seed, n, D, H, nh):
    return case_of(node_problem(seed, n, D, H, nh))


@functools.lru_cache(maxsize=3)
def edge_case(seed, ne, n, D, H, nh, graph="general"):
    return case_of(edge_problem(seed, ne, n, D, H, nh, graph))


@functools.lru_cache(maxsize=3)
def projection_case(seed, n, D, H):
    return case_of(projection_problem(seed, n, D, H))


# ---- guards -----------------------------------------------------------------------------------------------------------------
CANARY_BYTE = 0xA5          # float32 0xA5A5A5A5 = -2.87e-16, bf16 / fp16 0xA5A5: finite, and no kernel produces rows of it
SPARE_ROWS = 40             # rows of canary behind every output: more than one 32-row tile


def guarded(x, device, ld=None, rows_around=SPARE_ROWS):
    """The matrix ``x`` as a row slice (row stride ``ld`` >= width) of a NaN-filled buffer on ``device``: NaN rows before and
    behind, NaN columns past the width.  Integer matrices (src / dst as [ne, 1]) are surrounded by -1: a row of NaN in front
    of a guarded table.  16-byte alignment of the first row is kept (rows_around * ld * 4 bytes)."""
    n, d = x.shape
    ld = d if ld is None else ld
    fill = float("nan") if x.is_floating_point() else -1
    return guarded_pair(x, device, ld, rows_around)[1]


def guarded_pair(x, device, ld=None, rows_around=SPARE_ROWS):
    """-> (buf, view) of :func:`guarded`, for kernels that write the guarded matrix in place."""
    n, d = x.shape
    ld = d if ld is None else ld
    fill = float("nan") if x.is_floating_point() else -1
    buf = torch.full((n + 2 * rows_around, ld), fill, dtype=x.dtype, device=device)
    view = buf[rows_around:rows_around + n, :d]
    view.copy_(x)
    return buf, view


def assert_guard_intact(buf, n, what, rows_around=SPARE_ROWS):
    """The NaN rows around an input that a kernel wrote in place (x_out is x, e_out is e_in) are still NaN."""
    assert bool(torch.isnan(buf[:rows_around]).all()) and bool(torch.isnan(buf[rows_around + n:]).all()), \
        f"{what}: rows outside the matrix were written"


def canary_buffer(rows, width, dtype, device):
    buf = torch.empty((rows, width), dtype=dtype, device=device)
    buf.view(torch.uint8).fill_(CANARY_BYTE)
    return buf


def canary_output(n, width, device, ld=None, rows_before=0, rows_behind=SPARE_ROWS, dtype=torch.float32):
    """-> (buf, view): ``view`` [n, width] (row stride ``ld``) inside a canary-filled ``buf`` with spare rows on both sides
    and spare columns where ld > width."""
    ld = width if ld is None else ld
    buf = canary_buffer(rows_before + n + rows_behind, ld, dtype, device)
    return buf, buf[rows_before:rows_before + n, :width]


def assert_canaries(buf, written_rows, width, what):
    """Every byte of ``buf`` outside rows ``written_rows`` = (first, end) x columns [0, width) still holds the canary."""
    first, end = written_rows
    alive = buf.view(torch.uint8).reshape(buf.shape[0], -1) == CANARY_BYTE
    esize = buf.element_size()
    alive[first:end, :width * esize] = True
    if not bool(alive.all()):
        r, c = (int(v) for v in (~alive).nonzero()[0])
        raise AssertionError(f"{what}: canary overwritten at row {r} (the output ends at row {end}), element {c // esize} "
                             f"(the output is {width} wide)")
