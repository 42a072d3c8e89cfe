"""Problems and gates for the backward kernels (cgnn_mlp_backward, cgnn_edge_mlp_backward, cgnn_linear2_rows) that can see
ONE wrong row among 10^5, at sizes where a wave of the persistent tile loop takes a second tile (test infrastructure, in
the style of edge_checks.py).

* ``rows_past_one_pass(passes)``: the smallest row count at which every wave of ``grid_for_tiles`` / ``tile_range()``
  (csrc/runtime.hip, csrc/cgnn_common.hpp, restated here and checked exhaustively on the CPU) runs at least ``passes``
  tiles, some one more, with a tile count that is no multiple of 8 and a ragged last tile.
* ``mlp_problem`` / ``edge_problem`` / ``linear2_problem``: seeded problems whose rows span the value scales of training:
  ``dy`` rows x 10^(-8 U) (a mean-reduced loss over 10^6 particles gives 1e-8), input rows with one block x 1e-3 and one
  x 30.  A ReLU whose float64 pre-activation lies at rounding distance from zero makes the gradient of its row
  discontinuous: ANY f32 evaluation may take the other branch and move that row by about 1 / sqrt(H).  Such rows
  (min |a| / max |a| <= 1e-5 over a hidden layer, 100 x the f32 error of a pre-activation) are re-drawn from the same
  generator until none is left (at most 2 % of the rows, asserted); nothing is excluded from any gate afterwards.
* gates against float64 autograd: parameters ``max |err| <= 2e-5 max |want|`` per tensor (sums over all rows: the tensor
  norm is the right one; 1.5 x at width 256 as everywhere in the project), every data gradient laid out in rows
  ``||got_row - want_row|| <= 2e-5 ||want_row||`` for EVERY row.  The same backward evaluated by torch in float32 on the
  CPU (the yardstick) has to meet a quarter of every gate, or the inputs are at fault and the problem is refused.
"""
import functools

import torch

import edge_checks as ec

GTOL = 2e-5                 # the project's gradient tolerance (tests/test_gpu_training.py)
FRAGILE = 1e-5              # min |a| / max |a| of a hidden layer's pre-activations at or below which a row is re-drawn
REDRAW_CAP = 0.02
# The float32 yardstick of an MLP runs autograd over this many rows at a time.  A BLAS may add the n terms of a thin product
# (dW of a 3-wide decoder: [3, n] x [n, 128]) one after the other, which costs eps sqrt(n) / 3 of the sum -- 1.2e-5 was measured
# at n = 131,239 on one CPU, 5.6e-7 on another, for the same inputs: the summation's error, not the inputs'.  In chunks of 1024
# that term is 11 x smaller whatever the BLAS does.
YARD_CHUNK = 1024


# ---- moved here from test_gpu_training.py / test_gpu_training_edge.py (shared with test_gpu_backward_gates.py) -------------
def max_norm_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-12)


def close(got, want, tol=GTOL):
    err = max_norm_err(got, want)
    if err > tol:
        print(f"close: max |got - want| / max |want| = {err:.3e} > {tol:.1e}")      # shown by pytest on failure
    return err <= tol


def rand_mlp(gen, fin, hid, out, nh, ln):
    dims = [fin] + [hid] * nh + [out]
    sd = {}
    for i in range(nh + 1):
        sd[f"m.0.{2 * i}.weight"] = (torch.rand(dims[i + 1], dims[i], generator=gen) * 2 - 1) / dims[i] ** 0.5
        sd[f"m.0.{2 * i}.bias"] = torch.rand(dims[i + 1], generator=gen) - 0.5
    if ln:
        sd["m.1.weight"] = 1 + 0.1 * torch.randn(out, generator=gen)
        sd["m.1.bias"] = 0.1 * torch.randn(out, generator=gen)
    return sd


def edge_sd(gen, D, H, nh):
    """An edge model: first Linear over cat[x[src], x[dst], e] (3 D columns), LayerNorm."""
    sd = rand_mlp(gen, 3 * D, H, D, nh, False)
    sd["m.1.weight"] = 1 + 0.1 * torch.randn(D, generator=gen)
    sd["m.1.bias"] = 0.1 * torch.randn(D, generator=gen)
    return sd


class Lin:   # what training._TrainMLP / _TrainEdge need from an nn.Linear / nn.LayerNorm
    def __init__(self, w, b):
        self.weight, self.bias = w, b


def edges(gen, n, graph, ne=None):
    """(src, dst, fixed_k): receiver-sorted fixed in-degree k ("k8", "k16", ...), or a general (unsorted, ragged) edge list
    (of ``ne`` edges, 5 n + 3 by default)."""
    if graph == "general":
        e = 5 * n + 3 if ne is None else ne
        return (torch.randint(0, n, (e,), generator=gen, dtype=torch.int32),
                torch.randint(0, n, (e,), generator=gen, dtype=torch.int32), 0)
    k = int(graph[1:])
    src = torch.randint(0, n, (n * k,), generator=gen, dtype=torch.int32)
    return src, torch.arange(n, dtype=torch.int32).repeat_interleave(k), k


def param_names(nh, ln=True):
    return [f"m.0.{2 * i}.{p}" for i in range(nh + 1) for p in ("weight", "bias")] + (["m.1.weight", "m.1.bias"] if ln else [])


# ---- the tile map of every persistent kernel, restated ---------------------------------------------------------------------
def grid_for_tiles(tiles, cus, blocks_per_cu=2, waves=4):
    """csrc/runtime.hip grid_for_tiles."""
    blocks = min((tiles + waves - 1) // waves, cus * blocks_per_cu)
    blocks = max(blocks, 1)
    if blocks >= 8:
        blocks = (blocks + 7) & ~7
    return blocks


def tile_range(tiles, nb, b, wave, waves):
    """csrc/cgnn_common.hpp tile_range(): the tiles wave ``wave`` of workgroup ``b`` of ``nb`` visits, as a range."""
    if nb % 8 == 0:
        xcd, slot, per = b & 7, b >> 3, nb >> 3
        return range(tiles * xcd // 8 + slot * waves + wave, tiles * (xcd + 1) // 8, per * waves)
    return range(b * waves + wave, tiles, nb * waves)


def tiles_per_wave(n, cus, waves=4):
    """-> (fewest, most) tiles any wave of the launch for ``n`` rows runs."""
    tiles = (n + 31) // 32
    nb = grid_for_tiles(tiles, cus, 2, waves)
    counts = [len(tile_range(tiles, nb, b, w, waves)) for b in range(nb) for w in range(waves)]
    return min(counts), max(counts)


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_runs_passes(n, passes=2, cus=None):
    """The launch for ``n`` rows has more tiles than ``passes - 1`` sweeps of the grid's 8 CUs wave slots, every wave
    runs at least ``passes`` tiles, some run one more, and the eighths of the tile range are uneven."""
    cus = device_cus() if cus is None else cus
    tiles = (n + 31) // 32
    assert tiles > 8 * cus * (passes - 1), (n, tiles, cus)
    lo, hi = tiles_per_wave(n, cus)
    assert lo >= passes and hi > lo and tiles % 8 != 0, (n, cus, lo, hi)
    return n


def rows_past_one_pass(passes=2, cus=None):
    cus = device_cus() if cus is None else cus
    n = 32 * (8 * cus * passes + 5) + 7                    # the last tile is ragged
    return assert_runs_passes(n, passes, cus)


def second_pass_tile(n, cus):
    """A tile that some wave reaches in its SECOND trip through the tile loop (the last tile of the first eighth)."""
    tiles = (n + 31) // 32
    nb = grid_for_tiles(tiles, cus)
    tr = tile_range(tiles, nb, 0, 0, 4)
    assert len(tr) >= 2
    return tr[1]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def row_scales(gen, n):
    """10^(-8 U), U uniform per row: 1e-8 .. 1."""
    return 10.0 ** (-8.0 * torch.rand(n, generator=gen))


def input_rows(gen, n, d):
    """-> (randn rows with one block of 50 rows x 1e-3 and one x 30 where n allows (edge_checks.node_rows), the factors)."""
    s = torch.ones(n)
    if n >= 200:
        s[60:110] = 1e-3
        s[130:180] = 30.0
    return torch.randn(n, d, generator=gen) * s[:, None], s


def fragile_rows(pre_activations):
    """Rows with min |a| / max |a| <= FRAGILE over any of the hidden layers' (float64) pre-activations."""
    bad = None
    for a in pre_activations:
        a = a.abs()
        b = a.min(dim=1).values <= FRAGILE * a.max(dim=1).values
        bad = b if bad is None else bad | b
    return bad


def _redraw(gen, rows, scales, pre_activations_of, cap=REDRAW_CAP):
    """Re-draw (in place, from ``gen``) every row of ``rows`` that :func:`fragile_rows` names, until none is left.
    ``pre_activations_of(idx)``: the hidden pre-activations of the rows ``idx`` in float64.  -> the number of re-draws
    (asserted <= ``cap`` of the rows when a cap is given)."""
    n = rows.shape[0]
    idx = torch.arange(n)
    total = 0
    for _ in range(64):
        idx = idx[fragile_rows(pre_activations_of(idx))]
        if idx.numel() == 0:
            break
        total += idx.numel()
        rows[idx] = torch.randn(idx.numel(), rows.shape[1], generator=gen) * scales[idx, None]
    else:
        raise AssertionError("fragile rows remain after 64 re-draws")
    assert cap is None or total <= cap * n, f"{total} of {n} rows re-drawn (cap {cap:.0%})"
    return total


def mlp_pre_activations(sd, u, nh):
    """Float64 pre-activations of the ``nh`` hidden layers of rand_mlp's ``m.0`` for the rows ``u``."""
    h, out = u.double(), []
    for i in range(nh):
        a = h @ sd[f"m.0.{2 * i}.weight"].double().t() + sd[f"m.0.{2 * i}.bias"].double()
        out.append(a)
        h = a.relu()
    return out


def redraw_fragile_mlp_rows(gen, sd, u, nh, scales=None, cap=REDRAW_CAP):
    scales = torch.ones(u.shape[0]) if scales is None else scales
    return _redraw(gen, u, scales, lambda idx: mlp_pre_activations(sd, u[idx], nh), cap)


def edge_pre_activations(sd, x, src, dst, e, nh, D):
    w0 = sd["m.0.0.weight"].double()
    xd = x.double()
    a = (xd @ w0[:, :D].t())[src.long()] + (xd @ w0[:, D:2 * D].t())[dst.long()] + e.double() @ w0[:, 2 * D:].t() \
        + sd["m.0.0.bias"].double()
    out = [a]
    for i in range(1, nh):
        a = a.relu() @ sd[f"m.0.{2 * i}.weight"].double().t() + sd[f"m.0.{2 * i}.bias"].double()
        out.append(a)
    return out


def redraw_fragile_edge_rows(gen, sd, x, src, dst, e, nh, scales=None, cap=REDRAW_CAP):
    scales = torch.ones(e.shape[0]) if scales is None else scales
    D = x.shape[1]
    return _redraw(gen, e, scales, lambda idx: edge_pre_activations(sd, x, src[idx], dst[idx], e[idx], nh, D), cap)


def mlp_problem(seed, n, fin, fin2, hid, out, nh, ln):
    """y = [LN](MLP(u)) with gradient dy: dict(sd, u, dy, dy_scale, redrawn, ...)."""
    gen = torch.Generator().manual_seed(seed)
    sd = rand_mlp(gen, fin + fin2, hid, out, nh, ln)
    u, s_in = input_rows(gen, n, fin + fin2)
    dy_scale = row_scales(gen, n)
    dy = torch.randn(n, out, generator=gen) * dy_scale[:, None]
    redrawn = redraw_fragile_mlp_rows(gen, sd, u, nh, s_in)
    return dict(sd=sd, u=u, dy=dy, dy_scale=dy_scale, redrawn=redrawn, n=n, fin=fin, fin2=fin2, hid=hid, out=out, nh=nh, ln=ln)


def edge_problem(seed, H, D, nh, graph, n, ne=None):
    """One round's edge update u = LN(MLP(cat[x[src], x[dst], e])) under L = <e + u, de_next> + <agg(u), d_agg>, on ``n``
    nodes (see :func:`edges` for the edge count)."""
    gen = torch.Generator().manual_seed(seed)
    src, dst, fixed_k = edges(gen, n, graph, ne)
    ne = src.numel()
    sd = edge_sd(gen, D, H, nh)
    x, _ = input_rows(gen, n, D)
    e, s_e = input_rows(gen, ne, D)
    de_next = torch.randn(ne, D, generator=gen) * row_scales(gen, ne)[:, None]
    d_agg = torch.randn(n, D, generator=gen) * row_scales(gen, n)[:, None]
    redrawn = redraw_fragile_edge_rows(gen, sd, x, src, dst, e, nh, s_e)
    return dict(sd=sd, x=x, e=e, src=src, dst=dst, fixed_k=fixed_k, de_next=de_next, d_agg=d_agg, redrawn=redrawn, n=n, ne=ne,
                H=H, D=D, nh=nh)


def linear2_problem(seed, n, K, O):
    """out = add1 + add2 + a Wa^T + b Wb^T with every row of a, b, add1, add2 x 10^(-8 U) (one factor per row)."""
    gen = torch.Generator().manual_seed(seed)
    wa = (torch.rand(O, K, generator=gen) * 2 - 1) / K ** 0.5
    wb = (torch.rand(O, K, generator=gen) * 2 - 1) / K ** 0.5
    s = row_scales(gen, n)[:, None]
    a, b = torch.randn(n, K, generator=gen) * s, torch.randn(n, K, generator=gen) * s
    add1, add2 = torch.randn(n, O, generator=gen) * s, torch.randn(n, O, generator=gen) * s
    return dict(wa=wa, wb=wb, a=a, b=b, add1=add1, add2=add2, n=n)


# ---- references: torch autograd on the CPU, float64 (the oracle) or float32 (the yardstick) -----------------------------------
def _mlp_forward(sd, h, nh, ln):
    for i in range(nh):
        h = torch.relu(torch.nn.functional.linear(h, sd[f"m.0.{2 * i}.weight"], sd[f"m.0.{2 * i}.bias"]))
    y = torch.nn.functional.linear(h, sd[f"m.0.{2 * nh}.weight"], sd[f"m.0.{2 * nh}.bias"])
    if ln:
        y = torch.nn.functional.layer_norm(y, (y.shape[-1],), sd["m.1.weight"], sd["m.1.bias"], 1e-5)
    return y


def mlp_reference(p, dtype=torch.float64, chunk=None):
    """-> dict(du [n, fin + fin2], grads in ``param_names`` order) by autograd in ``dtype`` (cpu_ref.mlp / mlp_ln's lines).
    ``chunk``: rows per backward call; the parameter gradients of the calls are added in ``dtype`` (autograd's ``+=``)."""
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p["sd"].items()}
    n = p["u"].shape[0]
    du = []
    for r0 in range(0, n, chunk or n):
        r1 = min(n, r0 + (chunk or n))
        u = p["u"][r0:r1].detach().to(dtype).clone().requires_grad_(True)
        _mlp_forward(sd, u, p["nh"], p["ln"]).backward(p["dy"][r0:r1].to(dtype))
        du.append(u.grad)
    return dict(du=torch.cat(du), grads=[sd[k].grad for k in param_names(p["nh"], p["ln"])])


def edge_reference(p, dtype=torch.float64):
    """-> dict(de, dx, dps, dpd, dy, grads).  The first Linear is evaluated as Ws x[src] + Wd x[dst] + We e + b1 (the same
    function as over cat[x[src], x[dst], e], without the [E, 3 D] matrix); dps / dpd are the sender / receiver sums of
    dL/dh1."""
    D, H, nh, n = p["D"], p["H"], p["nh"], p["n"]
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p["sd"].items()}
    x = p["x"].detach().to(dtype).clone().requires_grad_(True)
    e = p["e"].detach().to(dtype).clone().requires_grad_(True)
    src, dst = p["src"].long(), p["dst"].long()
    de_next, d_agg = p["de_next"].to(dtype), p["d_agg"].to(dtype)
    w0 = sd["m.0.0.weight"]
    h1 = (x @ w0[:, :D].t())[src] + (x @ w0[:, D:2 * D].t())[dst] + e @ w0[:, 2 * D:].t() + sd["m.0.0.bias"]
    h1.retain_grad()
    z = h1.relu()
    for i in range(1, nh + 1):
        z = torch.nn.functional.linear(z, sd[f"m.0.{2 * i}.weight"], sd[f"m.0.{2 * i}.bias"])
        if i < nh:
            z = z.relu()
    u = torch.nn.functional.layer_norm(z, (D,), sd["m.1.weight"], sd["m.1.bias"], 1e-5)
    agg = torch.zeros(n, D, dtype=dtype).index_add(0, dst, u)
    ((e + u) * de_next).sum().add((agg * d_agg).sum()).backward()
    zero = torch.zeros(n, H, dtype=dtype)
    return dict(de=e.grad, dx=x.grad, dps=zero.index_add(0, src, h1.grad), dpd=zero.index_add(0, dst, h1.grad),
                dy=de_next + d_agg[dst], grads=[sd[k].grad for k in param_names(nh)])


def linear2_reference(p, addends, dtype=torch.float64):
    out = p["a"].to(dtype) @ p["wa"].to(dtype).t() + p["b"].to(dtype) @ p["wb"].to(dtype).t()
    if addends >= 1:
        out = out + p["add1"].to(dtype)
    if addends >= 2:
        out = out + p["add2"].to(dtype)
    return out


# ---- gates ---------------------------------------------------------------------------------------------------------------
def param_tol(width):
    return GTOL if width <= 128 else 1.5 * GTOL


def row_err(got, want):
    """-> (max over rows of ||got_row - want_row|| / ||want_row||, the row) against a float64 ``want``."""
    return ec.row_rel_max(got.detach().cpu().double(), want.detach().double())


def assert_rows(got, want, what, tol=GTOL):
    """EVERY row: ||got_row - want_row|| <= tol ||want_row||.  -> the worst row's relative error."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst, where = row_err(got, want)
    assert worst <= tol, f"{what}: row {where} (tile {where // 32}) differs by {worst:.3e} of its norm (gate {tol:.1e})"
    return worst


def assert_params(grads, want, names, tol, what):
    """Every parameter gradient: max |err| <= tol max |want| of its tensor.  -> the worst tensor's error."""
    assert len(grads) == len(want) == len(names), what
    worst = 0.0
    for name, g, w in zip(names, grads, want):
        assert g.shape == w.shape, (what, name)
        err = max_norm_err(g, w)
        assert err <= tol, f"{what}: {name} max |err| / max |want| = {err:.3e} (gate {tol:.1e})"
        worst = max(worst, err)
    return worst


def _split(p, du):
    """du -> {"du1": ..., "du2": ...} by the problem's input split."""
    out = {"du1": du[:, :p["fin"]]}
    if p["fin2"]:
        out["du2"] = du[:, p["fin"]:]
    return out


def check_mlp(p, want, du1, du2, grads, what, frac=1.0):
    """All gates of an MLP backward against ``want`` (:func:`mlp_reference` in float64), each at ``frac`` of its
    tolerance.  -> dict(max_norm, row, param): the worst values."""
    got = {"du1": du1}
    if p["fin2"]:
        got["du2"] = du2
    ws = _split(p, want["du"])
    st = dict(max_norm=0.0, row=0.0, param=0.0)
    for k, g in got.items():
        st["max_norm"] = max(st["max_norm"], max_norm_err(g, ws[k]))
        st["row"] = max(st["row"], assert_rows(g, ws[k], f"{what} {k}", frac * GTOL))
    assert st["max_norm"] <= frac * GTOL, (what, st)
    st["param"] = assert_params(grads, want["grads"], param_names(p["nh"], p["ln"]), frac * param_tol(max(p["hid"], p["out"])),
                                what)
    return st


def check_edge(p, want, got, what, frac=1.0):
    """``got``: dict(de, dx, dps, dpd, grads) of an edge-round backward; every row-laid-out tensor per row, parameters per
    tensor, against :func:`edge_reference` in float64.  -> dict(max_norm, row, param)."""
    st = dict(max_norm=0.0, row=0.0, param=0.0)
    for k in ("de", "dps", "dpd", "dx"):
        st["max_norm"] = max(st["max_norm"], max_norm_err(got[k], want[k]))
        st["row"] = max(st["row"], assert_rows(got[k], want[k], f"{what} {k}", frac * GTOL))
    assert st["max_norm"] <= frac * GTOL, (what, st)
    st["param"] = assert_params(got["grads"], want["grads"], param_names(p["nh"]), frac * param_tol(p["D"]), what)
    return st


def report(what, st, yard=None):
    """One line per case for DESIGN.md section 7b (``pytest -s``)."""
    line = f"backward-gate {what}: max-norm {st['max_norm']:.2e} worst-row {st['row']:.2e} worst-param {st['param']:.2e}"
    if yard is not None:
        line += f" | float32 yardstick {yard['max_norm']:.2e} {yard['row']:.2e} {yard['param']:.2e}"
    print(line)


def with_spike(p, key, row, col, value):
    """A copy of problem ``p`` with one value of its input ``key`` ("u" / "e") replaced -- every other row keeps its bits --,
    refused if that makes the row fragile."""
    q = dict(p)
    q[key] = p[key].clone()
    q[key][row, col] = value
    if key == "u":
        a = mlp_pre_activations(q["sd"], q["u"][row:row + 1], q["nh"])
    else:
        a = edge_pre_activations(q["sd"], q["x"], q["src"][row:row + 1], q["dst"][row:row + 1], q["e"][row:row + 1], q["nh"], q["D"])
    assert not bool(fragile_rows(a).any()), "the spiked row is fragile: take another seed"
    return q


# ---- cases: the float64 oracle is computed once and shared by the tests (and pairings) that use a problem; treat as read-only --
def mlp_case_of(p):
    """-> (float64 reference, the float32 yardstick's worst values).  The yardstick -- torch float32 autograd on the CPU --
    has to meet a QUARTER of every gate: if it does not, the inputs are at fault, not a kernel."""
    want = mlp_reference(p)
    y = mlp_reference(p, torch.float32, YARD_CHUNK)
    ys = _split(p, y["du"])
    return want, check_mlp(p, want, ys["du1"], ys.get("du2"), y["grads"], "float32 yardstick", frac=0.25)


def edge_case_of(p):
    want = edge_reference(p)
    return want, check_edge(p, want, edge_reference(p, torch.float32), "float32 yardstick", frac=0.25)


@functools.lru_cache(maxsize=2)
def mlp_case(seed, n, fin, fin2, hid, out, nh, ln):
    """-> (problem, float64 reference, yardstick)."""
    p = mlp_problem(seed, n, fin, fin2, hid, out, nh, ln)
    return (p,) + mlp_case_of(p)


@functools.lru_cache(maxsize=2)
def edge_case(seed, H, D, nh, graph, n, ne=None):
    p = edge_problem(seed, H, D, nh, graph, n, ne)
    return (p,) + edge_case_of(p)


@functools.lru_cache(maxsize=2)
def linear2_case(seed, n, K, O):
    """-> (problem, [float64 reference with 0, 1, 2 addends]); the float32 evaluation meets a quarter of the row gate."""
    p = linear2_problem(seed, n, K, O)
    want = [linear2_reference(p, k) for k in range(3)]
    for k in range(3):
        assert_rows(linear2_reference(p, k, torch.float32), want[k], "float32 yardstick", 0.25 * GTOL)
    return p, want
