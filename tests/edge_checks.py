"""Gates for edge-latent matrices that can see ONE wrong 32-edge tile among millions (test infrastructure).

A whole-matrix relative L2 norm is blind to a bad tile: one wrong tile in 10^4 moves it by 1e-2 at most.  The gates here
are per ROW, evaluated on the device in chunks (the matrices are 8-33 GB at the BASELINE sizes):

* ``assert_rows_close(a, b, tol)``: max over rows of ||a_row - b_row|| / ||b_row|| <= tol, for two runs of the same
  arithmetic through different kernels (bf16 paths differ by rounding flips: a few 1e-3 per row; a row of a wrong tile
  differs by O(1));
* ``sample_rows(...)``: the rows a persistent tile loop is most likely to get wrong -- the last tiles of every
  workgroup's range (the kernels cut the tile range into eight XCD shares and stride through each), the final
  (possibly partial) tiles, plus uniformly random ones;
* ``emulate_edge_stream_rows(...)``: the bf16-operand / f32-accumulate arithmetic of the one-launch edge stream
  (reference graph_network.py:57,:89-90,:182 with the first Linear split into Ps[src] + Pd[dst] + We e), recomputed in
  torch for sampled rows from the SAME Ps / Pd tables the kernel consumed;
* ``assert_table_is_rounded_exact(...)``: every element of a Ps / Pd table holds the correctly rounded value of SOME f32
  evaluation of its dot product (no tuned number: the bound is the a-priori one of ``oracle.bf16_stream.emulate_project``);
* ``assert_update_matches_emulation(...)`` / ``assert_residual_is_f32_sum(...)``: the emulation gates applied to every
  row of one round's UPDATE ``u`` (on ``e_out`` the residual stream dilutes every relative measure), and ``e_out`` held
  element-wise to ``e_in + u`` within two f32 roundings;
* ``corrupted_tile(...)``: a context manager that overwrites one tile of a result in place (with its neighbour's values:
  right statistics, wrong edges) and restores it -- every gate is run against it once to prove it would fail.
"""
import contextlib

import numpy as np
import torch

# the bf16-operand arithmetic itself is part of the oracle (oracle/bf16_stream.py: reference citations, pinned against
# cpu_ref on the CPU in every run); this file keeps the gates
from oracle.bf16_stream import bf, dot_bf16, emulate_edge_stream_rows, fold_state_dict, s32_table_to_logical  # noqa: F401

# A tighter, measured rel-L2 gate on the update u was tried and does NOT fit: the emulation with float64 sums against
# the same emulation with torch float32 matmuls (reference against reference: accumulation-order noise, the bf16 rounding
# flips it causes included) measures up to 9.3e-5 .. 1.6e-4 on u, depending on the seeds, over the shapes of
# tests/test_gpu_bf16_kernels.py (539, 4133 and 80069 edges, every (hidden, latent) pair, 1..3 hidden layers; largest at
# 256-wide shapes with three hidden layers, where single rows move by 3e-3 and, at 539 edges, one such row sets the
# norm), times 10 for the matrix core's different order = 1.6e-3.  Truncating the activations instead of
# rounding them moves u by 3.0e-3 .. 3.3e-3; half of that is 1.5e-3 < 1.6e-3.  So the project's 2e-3 stands alone -- on
# u, where it does reject truncated activations (on e_out, diluted by the residual stream, it did not).


def row_rel_max(a: torch.Tensor, b: torch.Tensor, chunk: int = 1 << 20):
    """-> (max over rows of ||a_row - b_row|| / ||b_row||, the row it occurs at); rows of b with zero norm count with
    their absolute difference."""
    assert a.shape == b.shape and a.dim() == 2
    worst, where = 0.0, -1
    for r0 in range(0, a.shape[0], chunk):
        x, y = a[r0:r0 + chunk], b[r0:r0 + chunk]
        num = (x - y).float().norm(dim=1)
        den = y.float().norm(dim=1).clamp_min(1e-30)
        rel = num / den
        rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
        m, i = rel.max(dim=0)
        if float(m) > worst or where < 0:
            worst, where = float(m), r0 + int(i)
    return worst, where


def assert_rows_close(a, b, tol, what="edge latents"):
    worst, where = row_rel_max(a, b)
    assert worst <= tol, f"{what}: row {where} (tile {where // 32}) differs by {worst:.3e} relative (gate {tol:.1e})"


def sample_rows(num_edges: int, n_random: int = 4096, seed: int = 0, device="cuda", tail_pairs: int = 256):
    """Row indices: two rows of every tile among the last ``tail_pairs`` tile PAIRS of each eighth of the pair range
    (covers the last iteration of every wave of a grid of up to 8 * tail_pairs / waves workgroups, for kernels that
    stride through eighths in pairs or in single tiles), all rows of the last two tiles, ``n_random`` random rows."""
    tiles = (num_edges + 31) // 32
    pairs = (tiles + 1) // 2
    picks = []
    for x in range(8):
        end = pairs * (x + 1) // 8
        lo = max(pairs * x // 8, end - tail_pairs)
        t = torch.arange(2 * lo, min(2 * end, tiles), dtype=torch.int64)
        picks += [t * 32 + 3, t * 32 + 29]
    picks.append(torch.arange(max(0, (tiles - 2) * 32), num_edges, dtype=torch.int64))
    gen = torch.Generator().manual_seed(seed)
    picks.append(torch.randint(0, num_edges, (n_random,), generator=gen, dtype=torch.int64))
    rows = torch.unique(torch.cat(picks))
    return rows[rows < num_edges].to(device)


def assert_rows_match_emulation(got_rows: torch.Tensor, want_rows: torch.Tensor, rows: torch.Tensor, what="edge latents"):
    """Per sampled row: max-abs <= 1e-2 x the sample's scale (a bf16 rounding flip in a hidden layer moves one value by
    a few 1e-3 of the scale; a wrong bias / LayerNorm vector / fragment / tile moves whole rows by O(scale))."""
    scale = float(want_rows.abs().max())
    err = (got_rows - want_rows).abs().max(dim=1).values
    worst, i = err.max(dim=0)
    assert float(worst) <= 1e-2 * scale, (f"{what}: edge row {int(rows[int(i)])} (tile {int(rows[int(i)]) // 32}) is off by "
                                          f"{float(worst):.3e}, scale {scale:.3e}")
    assert float((got_rows - want_rows).norm() / want_rows.norm()) <= 2e-3, what


def _ordered(t: torch.Tensor) -> torch.Tensor:
    """16-bit floats (bf16 / fp16: sign and magnitude) -> integers in the order of their values; +0 and -0 both 0."""
    bits = t.contiguous().view(torch.int16).to(torch.int32)
    mag = bits & 0x7FFF
    return torch.where(bits < 0, -mag, mag)


def _from_ordered(k: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    bits = torch.where(k < 0, k.abs() | 0x8000, k)
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    return bits.view(dtype)


def table_gate_failures(got: torch.Tensor, exact: torch.Tensor, bound: torch.Tensor, dtype: torch.dtype):
    """-> (boolean mask of the elements outside the gate of :func:`assert_table_is_rounded_exact`, number of elements
    that differ from the correctly rounded float64 value)."""
    assert got.shape == exact.shape == bound.shape and exact.dtype == torch.float64 and bound.dtype == torch.float64
    got64 = got.double()
    finite = torch.isfinite(got64)
    kg = _ordered(got64.float().to(dtype))
    representable = _from_ordered(kg, dtype).double() == got64
    # `got` is what every s in [(got + below) / 2, (got + above) / 2] rounds to (below / above: its neighbours in `dtype`);
    # some f32 evaluation may lie anywhere in [exact - bound, exact + bound]: the two intervals must meet.  Where bound is
    # below half a unit of `dtype` (everywhere but at sums that cancel to almost nothing) this is: got == round(exact), or
    # got is its neighbour and exact lies within bound of the midpoint between the two.
    lo_mid = 0.5 * (got64 + _from_ordered(kg - 1, dtype).double())
    hi_mid = 0.5 * (got64 + _from_ordered(kg + 1, dtype).double())
    meets = (exact + bound >= lo_mid) & (exact - bound <= hi_mid)
    ok = finite & representable & meets
    # for the report: elements that are not the value of `dtype` nearest to `exact` (torch rounds float64 through
    # float32, a double rounding: take the nearest of that value and its two neighbours)
    k0 = _ordered(exact.float().to(dtype))
    cands = torch.stack([_from_ordered(k0 + j, dtype).double() for j in (-1, 0, 1)])
    dist = (cands - exact).abs()
    dist = torch.where(torch.isfinite(cands), dist, torch.full_like(dist, float("inf")))
    same = got64 == cands.gather(0, dist.argmin(dim=0, keepdim=True))[0]          # +0 == -0
    return ~ok, int((~same).sum())


def assert_table_is_rounded_exact(got: torch.Tensor, exact: torch.Tensor, bound: torch.Tensor, dtype: torch.dtype,
                                  what: str = "table"):
    """``got`` (logical order, the table's values widened to float) holds, in EVERY element, the value of ``dtype``
    nearest to some f32 evaluation of the sum whose float64 value is ``exact`` and whose f32 evaluations all lie within
    ``bound`` of it: either ``got == round(exact)``, or ``got`` is the neighbouring value of ``dtype`` and ``exact`` lies
    within ``bound`` of the midpoint between the two (where an f32 sum may fall on the other side); in general, where a
    sum cancels so far that ``bound`` exceeds a unit of ``dtype`` at the result, the values that round to ``got`` must
    meet [exact - bound, exact + bound].  +0 and -0 are equal.
    -> the number of elements that differ from round(exact) (all of them inside the bound)."""
    bad, differ = table_gate_failures(got, exact, bound, dtype)
    nbad = int(bad.sum())
    if nbad:
        i = int(bad.flatten().nonzero()[0])
        r, c = divmod(i, got.shape[-1])
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements ({nbad / got.numel():.2%}) are not the rounded sum; first "
                             f"at row {r}, feature {c}: got {float(got.flatten()[i])!r}, exact {float(exact.flatten()[i])!r}, "
                             f"bound {float(bound.flatten()[i]):.3e}")
    return differ


def update_stats(got: torch.Tensor, want: torch.Tensor):
    """-> dict(max_abs / scale, rel_l2, row_rel): the three measures of :func:`assert_update_matches_emulation`."""
    scale = float(want.abs().max())
    return dict(max_abs=float((got - want).abs().max()) / scale,
                rel_l2=float((got.double() - want.double()).norm() / want.double().norm()),
                row_rel=row_rel_max(got, want)[0])


def assert_update_matches_emulation(got: torch.Tensor, want: torch.Tensor, what="edge update", l2_gate=None):
    """ALL rows of an update matrix ``u`` against its emulation: the project's emulation gates
    (:func:`assert_rows_match_emulation`: per-row max-abs <= 1e-2 x scale, rel-L2 <= 2e-3; per-row relative norm <= 1e-2
    as for the 256-wide edge encoder).  ``l2_gate``: another rel-L2 gate in place of the 2e-3 (5e-3 for LayerNorm inputs with a large mean, as test_edge_stream_layernorm_rows_with_a_large_mean),
    with the same max-abs gate.  -> :func:`update_stats`."""
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    st = update_stats(got, want)
    if l2_gate is None:
        assert_rows_match_emulation(got, want, torch.arange(got.shape[0]), what)
    else:
        assert st["max_abs"] <= 1e-2, f"{what}: max-abs {st['max_abs']:.3e} of the scale"
        assert st["rel_l2"] <= l2_gate, f"{what}: rel-L2 {st['rel_l2']:.3e} (gate {l2_gate:.1e})"
        return st
    assert_rows_close(got, want, 1e-2, what)
    return st


def assert_residual_is_f32_sum(e_out: torch.Tensor, e_in: torch.Tensor, e_upd: torch.Tensor, what="e_out"):
    """|e_out - (e_in + e_upd)| <= 2^-22 max(|e_in|, |e_upd|) in every element: two f32 roundings."""
    err = (e_out.double() - (e_in.double() + e_upd.double())).abs()
    excess = err - 2.0 ** -22 * torch.maximum(e_in.abs(), e_upd.abs()).double()
    assert float(excess.max()) <= 0.0, f"{what}: off by {float(err.max()):.3e} from e_in + e_upd (row {int(excess.max(dim=1).values.argmax())})"


@contextlib.contextmanager
def corrupted_tile(rows_matrix: torch.Tensor, tile: int):
    """Inside the block, tile ``tile`` (32 rows) of the row-major matrix holds the NEXT tile's values (or the previous
    one's for the last tile): plausible numbers on the wrong edges, what a wrong tile index or a stale register tile
    produces.  Restored afterwards."""
    n = rows_matrix.shape[0]
    r0, r1 = tile * 32, min(tile * 32 + 32, n)
    other = r1 if r1 + (r1 - r0) <= n else r0 - 32
    assert other >= 0
    saved = rows_matrix[r0:r1].clone()
    rows_matrix[r0:r1] = rows_matrix[other:other + (r1 - r0)].clone()
    try:
        yield
    finally:
        rows_matrix[r0:r1] = saved


def must_fail(fn, *args, **kwargs):
    """The gate ``fn`` has to reject its (corrupted) arguments."""
    try:
        fn(*args, **kwargs)
    except AssertionError:
        return
    raise AssertionError(f"{getattr(fn, '__name__', fn)} did not notice a deliberately corrupted tile")


# ---- seeded problems in the project's style, shared by the CPU test of the gates and the GPU tests ------------------
PAIRS = [(32, 32), (64, 64), (128, 128), (256, 256), (128, 64), (128, 256)]     # compiled (hidden, latent) pairs


def rand_linear(gen, out_dim, in_dim, fan_in=None):
    bound = 1.0 / np.sqrt(fan_in or in_dim)
    return ((torch.rand(out_dim, in_dim, generator=gen) * 2 - 1) * bound, (torch.rand(out_dim, generator=gen) * 2 - 1) * bound)


def rand_layer_norm(gen, d):
    return 1 + 0.1 * torch.randn(d, generator=gen), 0.1 * torch.randn(d, generator=gen)


def node_rows(gen, n, d):
    """x = 3 randn with one block of 50 rows scaled by 1e-3 and one by 30 (where n allows)."""
    x = 3 * torch.randn(n, d, generator=gen)
    if n >= 200:
        x[60:110] *= 1e-3
        x[130:180] *= 30
    return x


def projection_problem(seed, hidden, latent, n):
    """-> x [n, latent], (ws, None), (wd, b1): the sender / receiver column blocks of an edge model's first Linear."""
    gen = torch.Generator().manual_seed(seed)
    w1, b1 = rand_linear(gen, hidden, 3 * latent)
    return node_rows(gen, n, latent), w1[:, :latent].contiguous(), w1[:, latent:2 * latent].contiguous(), b1


def edge_problem(seed, hidden, latent, nh, num_edges, n=None, graph="random"):
    """One round's edge update on logical tables: dict(ps, pd, src, dst, e, lins, ln, b1, pd_raw).  ps / pd are
    bf16-representable random values (pd = bf(pd_raw + b1): the layer-0 bias lives in Pd); lins[0] = (We, None)."""
    gen = torch.Generator().manual_seed(seed)
    n = max(1, num_edges // 8) if n is None else n
    we, b1 = rand_linear(gen, hidden, latent, 3 * latent)
    lins = [(we, None)] + [rand_linear(gen, hidden, hidden) for _ in range(nh - 1)] + [rand_linear(gen, latent, hidden)]
    ln = rand_layer_norm(gen, latent)              # every parameter before anything sized by the graph: one seed, one model
    ps, pd_raw = torch.randn(n, hidden, generator=gen), torch.randn(n, hidden, generator=gen)
    if graph == "random":
        src = torch.randint(0, n, (num_edges,), generator=gen, dtype=torch.int32)
        dst = torch.randint(0, n, (num_edges,), generator=gen, dtype=torch.int32)
    else:                                                  # every edge from the last node to the first
        src = torch.full((num_edges,), n - 1, dtype=torch.int32)
        dst = torch.zeros(num_edges, dtype=torch.int32)
    return dict(ps=bf(ps), pd=bf(pd_raw + b1), pd_raw=pd_raw, b1=b1, src=src, dst=dst, lins=lins,
                ln=ln, e=3 * torch.randn(num_edges, latent, generator=gen))


def encoder_problem(seed, fin, hidden, latent, nh, n):
    gen = torch.Generator().manual_seed(seed)
    dims = [fin] + [hidden] * nh + [latent]
    lins = [rand_linear(gen, dims[i + 1], dims[i]) for i in range(nh + 1)]
    return dict(lins=lins, ln=rand_layer_norm(gen, latent), attr=torch.randn(n, fin, generator=gen))
