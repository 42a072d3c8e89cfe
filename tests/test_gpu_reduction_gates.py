"""GPU: the parameter-gradient reductions gated EXACTLY (tests/reduction_checks.py; the gates are tested on themselves in
tests/test_reduction_gates_cpu.py).  With small integers in g and a every product and every partial sum is a float32
integer, so the f32 MFMA, the three bf16 terms and the float atomics all have to give the integer reference's bits: one row
left out, one partial taken twice, one stale workspace slot or one value read from outside the operands (NaN) fails.  Every
case runs with a NaN-filled workspace and a guard region behind its reported size, twice into pre-filled outputs that are
wider and longer than the block written (canaries), on operands with NaN rows beyond n and NaN columns up to the leading
dimension.  The sizes come from the branch finders, and each test asserts from the restated partition that the branch is
entered.  Arithmetic (rounding, not indexing) is gated per element at 64 rows against torch's float32 product."""
import functools

import pytest
import torch

import reduction_checks as rc
from cosmology_gnn_simulation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poison_cached_workspaces():
    """The workspaces ``ops`` keeps per stream hold the previous call's partials: make them NaN (bytes 0xff)."""
    for ws in list(ops._WGRAD_WORKSPACE.values()) + list(ops._COLDOT_WORKSPACE.values()):
        ws.fill_(255)


# ---- weight gradients ----------------------------------------------------------------------------------------------------------
def _wgrad_run(form, p, with_db, calls=2):
    """``calls`` accumulations through ``form`` -> (dw, db) padded tensors; the workspace is NaN, its guard is checked."""
    lib = _lib.load()
    g, a, n, o, i = p["g"], p["a"], p["n"], p["out_dim"], p["in_dim"]
    dw, db = p["dw0"].clone(), p["db0"].clone()
    dw_k, db_k = dw[p["dw_rows"]], (db[p["db_span"]] if with_db else None)
    assert dw_k.is_contiguous() and dw_k.shape == (o, p["ld_dw"])
    dbp = None if db_k is None else db_k.data_ptr()
    ws = floats = None
    if form in ("ordered", "x3"):
        nbytes = lib.cgnn_weight_grad_workspace_bytes(n, o, i) if form == "ordered" else lib.cgnn_weight_grad_x3_workspace_bytes()
        ws, floats = rc.guarded_workspace(nbytes, DEV)
    for _ in range(calls):
        if form == "ordered":
            ws[:floats] = rc.NAN
            code = lib.cgnn_weight_grad_ordered(g.ptr, g.ld, o, a.ptr, a.ld, i, n, dw_k.data_ptr(), p["ld_dw"], p["col0"], dbp,
                                                ws.data_ptr(), 4 * floats, _stream())
        elif form == "atomic":
            code = lib.cgnn_weight_grad(g.ptr, g.ld, o, a.ptr, a.ld, i, n, dw_k.data_ptr(), p["ld_dw"], p["col0"], dbp, _stream())
        elif form == "x3":
            ws[:floats] = rc.NAN
            code = lib.cgnn_weight_grad_x3(g.ptr, g.ld, a.ptr, a.ld, n, dw_k.data_ptr(), p["ld_dw"], p["col0"], dbp,
                                           ws.data_ptr(), 4 * floats, _stream())
        else:                                   # "ops" / "ops_x3": the wrapper takes a contiguous a (column 0 of its tensor)
            assert a.col == 0
            _poison_cached_workspaces()
            ops.weight_grad(g.full[:, g.col:], g.ld, o, a.full, i, n, dw_k, p["col0"], db_k, "fp32x3" if form == "ops_x3" else "fp32")
            code = 0
        assert code == 0, (form, lib.cgnn_last_error())
    torch.cuda.synchronize()
    if ws is not None:
        rc.assert_guard(ws, floats, form)
    return dw, db


def _wgrad_check(form, p, with_db, what, calls=2):
    dw, db = _wgrad_run(form, p, with_db, calls)
    want_dw, want_db = rc.wgrad_expected(p, calls, with_db)
    rc.assert_exact(dw, want_dw, f"{what} {form} dw", rc.wgrad_block(p))
    rc.assert_exact(db, want_db, f"{what} {form} db", p["db_span"])


N7, N8, N9 = (rc.wgrad_n_for_chunks(c, 160, 64) for c in (7, 8, 9))        # the eight reduce lanes: one short, full, a second trip
N_CAPPED = rc.wgrad_smallest_capped_n(256, 256) + 8                       # 262153: chunks of 1032 rows, fewer than the cap

# (n, out_dim, in_dim, col0, extra columns of ld_g over the padded width, db, g_exp, a_exp)
ORDERED = [
    (1, 128, 17, 0, 0, True, 0, 0),              # the encoder's first Linear; G = 1, ragged tile
    (7, 3, 128, 3, 8, True, 0, 0),               # the decoder's last Linear
    (8, 1, 128, 128, 0, False, 0, 0),            # a one-wide head
    (9, 128, 256, 0, 0, True, 0, 0),             # the node model's first Linear, latent 128: 4 x 2 items
    (1023, 256, 256, 128, 0, True, 0, 0),        # latent 256: 16 items
    (1024, 31, 32, 0, 5, False, 0, 0),           # G = 1, full tile
    (1025, 32, 33, 3, 0, True, 0, 0),            # G = 2, full group with a ragged tile
    (2049, 33, 64, 0, 0, True, 0, 0),            # G = 2, full
    (N7, 96, 17, 3, 0, True, 0, 0),              # 3 items (a ragged workgroup of waves), 7 chunks
    (N8, 160, 32, 0, 3, True, 0, 0),             # 5 items: blockIdx.y 1 holds one wave; 8 chunks
    (N9, 160, 64, 128, 0, False, 0, 0),          # 5 items, G = 2; 9 chunks
    (1025, 96, 96, 0, 0, True, 0, 0),            # G = 2, PARTIAL last group (3 tiles), 6 items
    (2049, 33, 97, 3, 0, True, 0, 0),            # G = 4, full group with a ragged tile
    (1023, 3, 160, 0, 0, True, 0, 0),            # G = 4, partial last group: 1 tile of 4
    (9, 160, 224, 3, 32, True, 0, 0),            # G = 4, partial last group: 3 tiles of 4; 10 items
    (1025, 1, 1, 0, 0, True, 0, 0),
    (2049, 128, 128, 128, 0, True, -30, 10),     # g x 2^-30, a x 2^10: still exact in f32
    (N_CAPPED, 256, 256, 0, 0, True, 0, 0),      # the capped branch of wgrad_ordered_shape
]


def test_the_ordered_cases_hold_what_they_are_meant_to():
    """The case table against the restated partition: G = 1, 2, 4 each with a full and a partial (ragged) last group, item
    counts of 3, 5 and more than 8, 7 / 8 / 9 chunks, one capped case."""
    items = [rc.wgrad_items(o, i) for _, o, i, *_ in ORDERED]
    for G in (1, 2, 4):
        assert any(it["G"] == G and not it["partial_group"] for it in items)
    assert {it["G"] for it in items if it["partial_group"]} == {2, 4}
    assert {1, 17, 32, 33, 64, 96, 97, 128, 160, 224, 256} == {i for _, _, i, *_ in ORDERED}
    assert {1, 3, 31, 32, 33, 96, 128, 160, 256} == {o for _, o, *_ in ORDERED}
    assert {3, 5} <= {it["n_items"] for it in items} and any(it["n_items"] > 8 and it["ragged_items"] for it in items)
    assert {1, 7, 8, 9, 1023, 1024, 1025, 2049} <= {c[0] for c in ORDERED}
    assert [rc.wgrad_ordered_shape(n, o, i)[0] for n, o, i, *_ in ORDERED if n in (N7, N8, N9)] == [7, 8, 9]
    chunks, rows, _, _ = rc.wgrad_ordered_shape(N_CAPPED, 256, 256)
    assert rows > rc.WGRAD_ROWS and chunks < rc.wgrad_cap(256, 256) and N_CAPPED % 8 and N_CAPPED % rows % 8
    assert all(rc.wgrad_ordered_shape(n, o, i)[1] <= rc.WGRAD_ROWS for n, o, i, *_ in ORDERED[:-1])
    assert {0, 3, 128} == {c[3] for c in ORDERED}


@pytest.mark.parametrize("case", ORDERED, ids=lambda c: f"n{c[0]}-{c[1]}x{c[2]}-col{c[3]}")
def test_weight_grad_f32_forms_are_exact(case):
    """cgnn_weight_grad_ordered, cgnn_weight_grad (atomics) and ops.weight_grad on the same exact problem."""
    n, o, i, col0, ldg_extra, with_db, ge, ae = case
    p = rc.wgrad_problem(n + o, n, o, i, ld_g=(o + 31) // 32 * 32 + ldg_extra, col0=col0, g_exp=ge, a_exp=ae, device=DEV)
    assert p["g"].ld > o or o % 32 == 0
    assert p["a"].ld > i and p["ld_dw"] > col0 + i and p["g"].full.shape[0] >= n + 32
    lib = _lib.load()
    assert lib.cgnn_weight_grad_workspace_bytes(n, o, i) == rc.wgrad_workspace_bytes(n, o, i)
    for form in ("ordered", "atomic", "ops"):
        _wgrad_check(form, p, with_db, f"n={n} {o}x{i}")
    if not with_db:
        return
    _wgrad_check("ordered", p, False, f"n={n} {o}x{i} db NULL")          # and the bias sums leave db alone when it is NULL


# way: what the last live wave does (reduction_checks.x3_way); (n, way, ld, operand column, col0, g_exp, a_exp)
X3_FULL_TAIL = rc.x3_smallest_n("full_then_tail")
X3_FULL_ONLY = rc.x3_smallest_n("full_only")
X3_BIG = rc.x3_smallest_n("full_then_tail", start=300_000, min_full=3)
X3 = [
    (rc.x3_smallest_n("tail_only"), "tail_only", 128, 0, 0, 0, 0),
    (15, "tail_only", 136, 4, 128, 0, 0),
    (16, "full_only", 128, 0, 0, -100, 0),
    (17, "tail_only", 136, 4, 0, 0, 0),
    (X3_FULL_ONLY - 1, "tail_only", 128, 0, 128, 0, 0),
    (X3_FULL_ONLY, "full_only", 136, 4, 0, 0, 0),
    (X3_FULL_ONLY + 1, "tail_only", 128, 0, 0, -30, 10),
    (X3_FULL_TAIL, "full_then_tail", 128, 0, 128, 0, 0),
    (X3_FULL_TAIL, "full_then_tail", 136, 4, 0, -100, 0),
    (32 * 1024 + 16 * 3 + 5, "full_then_tail", 136, 4, 128, 0, 0),
    (X3_BIG, "full_then_tail", 128, 0, 0, 0, 0),
]


@pytest.mark.parametrize("case", X3, ids=lambda c: f"n{c[0]}-{c[1]}-ld{c[2]}-col{c[4]}-e{c[5]}")
def test_weight_grad_x3_is_exact_on_every_way_through_its_row_loop(case):
    n, way, ld, col, col0, ge, ae = case
    assert rc.x3_way(n) == way
    part = rc.x3_partition(n)
    if n in (X3_FULL_TAIL, X3_BIG):
        assert part["rows_per_wave"] >= 32 and part["last_full"] >= (3 if n == X3_BIG else 1) and 1 <= part["last_tail"] <= 15
    if n == X3_FULL_ONLY:
        assert part["idle"] == 0
    p = rc.wgrad_problem(3 * n + col0, n, 128, 128, ld_g=ld - col, ld_a=ld - col, g_col=col, a_col=col, col0=col0, g_exp=ge,
                         a_exp=ae, device=DEV)
    assert p["g"].ld == p["a"].ld == ld and p["g"].ptr % 16 == 0 and p["a"].ptr % 16 == 0 and p["g"].col == col
    _wgrad_check("x3", p, True, f"n={n}")
    _wgrad_check("x3", p, False, f"n={n} db NULL")
    if col == 0:
        _wgrad_check("ops_x3", p, True, f"n={n}")


@pytest.mark.parametrize("n", [17, X3_FULL_TAIL])
def test_ops_routes_a_misaligned_g_to_the_ordered_kernel_with_the_same_exact_result(n):
    """g starts one float into its rows: 16-byte loads are impossible, ops.weight_grad(precision="fp32x3") takes
    cgnn_weight_grad_ordered, the C entry itself refuses -- and the result has the same bits."""
    p = rc.wgrad_problem(n, n, 128, 128, ld_g=131, ld_a=128, g_col=1, col0=128, device=DEV)
    assert p["g"].ptr % 16 == 4 and p["g"].ld % 4 == 0
    lib = _lib.load()
    ws, floats = rc.guarded_workspace(lib.cgnn_weight_grad_x3_workspace_bytes(), DEV)
    dw = p["dw0"].clone()
    code = lib.cgnn_weight_grad_x3(p["g"].ptr, p["g"].ld, p["a"].ptr, p["a"].ld, n, dw[p["dw_rows"]].data_ptr(), p["ld_dw"], 128,
                                   None, ws.data_ptr(), 4 * floats, _stream())
    torch.cuda.synchronize()
    assert code == -2 and torch.equal(dw, p["dw0"])
    _wgrad_check("ops_x3", p, True, f"misaligned g n={n}")


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("name", sorted(rc.PROBES))
def test_weight_grad_x3_takes_each_of_its_six_products(name, n):
    """The term probes: results that are float32 values at every partial sum and cannot be had without the products
    ``needs`` (tests/test_reduction_gates_cpu.py removes each and sees other bits)."""
    for col0 in (0, 128):
        p = rc.probe_problem(name, n, col0, DEV)
        _wgrad_check("x3", p, False, f"probe {name} n={n} col0={col0}", calls=1)


# ---- column sums ---------------------------------------------------------------------------------------------------------------
# (n, width, ld_a, ld_b, column of a, column of b, 16-byte loads)
COLDOT = [
    (1, 1, 8, 5, 0, 0, False),
    (255, 3, 4, 8, 0, 0, False),
    (256, 4, 8, 12, 0, 0, True),
    (257, 5, 9, 8, 0, 0, False),
    (511, 20, 24, 32, 0, 0, True),               # 5 column groups on 8 lanes: idle column lanes, 16-byte loads
    (512, 64, 68, 72, 0, 0, True),
    (513, 128, 132, 136, 0, 0, True),
    (4 * 512 + 1, 252, 256, 260, 0, 0, True),     # 63 groups
    (9 * 512 - 1, 256, 260, 264, 0, 0, True),
    (257, 260, 264, 268, 0, 0, True),            # two column passes: 64 groups, then 1 (256 row lanes)
    (513, 516, 520, 524, 4, 0, True),            # three passes; a off its row start, still aligned
    (4 * 512 + 1, 64, 68, 72, 1, 0, False),       # width % 4 == 0 on the scalar path: a's pointer is off by one float
    (513, 128, 131, 136, 0, 0, False),           # ... an odd leading dimension
    (9 * 512 - 1, 20, 24, 32, 0, 1, False),      # ... b's pointer
]


def _col_dot_run(form, p, which):
    """-> the padded outputs (out_ab | out_s, out_a | None) after two accumulations.  ``which``: "ab" (b present), "s" (b NULL),
    "both" (the two-sum form)."""
    lib = _lib.load()
    a, b, n, w = p["a"], p["b"], p["n"], p["width"]
    o1, o2 = p["out0"].clone(), (p["out0"].clone() if which == "both" else None)
    k1, k2 = o1[p["span"]], (None if o2 is None else o2[p["span"]])
    bp, ldb = (None, 0) if which == "s" else (b.ptr, b.ld)
    ws = floats = None
    if form == "ordered":
        ws, floats = rc.guarded_workspace(lib.cgnn_col_dot_workspace_bytes(n, w), DEV)
    for _ in range(2):
        if form == "ordered":
            ws[:floats] = rc.NAN
            code = lib.cgnn_col_dot_ordered(a.ptr, a.ld, bp, ldb, n, w, k1.data_ptr(), None if k2 is None else k2.data_ptr(),
                                            ws.data_ptr(), 4 * floats, _stream())
        elif form == "atomic":
            code = (lib.cgnn_col_dot2(a.ptr, a.ld, bp, ldb, n, w, k1.data_ptr(), k2.data_ptr(), _stream()) if which == "both" else
                    lib.cgnn_col_dot(a.ptr, a.ld, bp, ldb, n, w, k1.data_ptr(), _stream()))
        else:
            _poison_cached_workspaces()
            av, bv = a.full[:, a.col:], b.full[:, b.col:]
            if which == "both":
                ops.col_dot2(av, a.ld, bv, b.ld, n, w, k1, k2)
            else:
                ops.col_dot(av, a.ld, None if which == "s" else bv, ldb, n, w, k1)
            code = 0
        assert code == 0, (form, which, lib.cgnn_last_error())
    torch.cuda.synchronize()
    if ws is not None:
        rc.assert_guard(ws, floats, f"col_dot {form} {which}")
    return o1, o2


@pytest.mark.parametrize("case", COLDOT, ids=lambda c: f"n{c[0]}-w{c[1]}-ld{c[2]}+{c[4]}-{c[3]}+{c[5]}")
def test_col_dot_forms_are_exact(case):
    n, w, ld_a, ld_b, ca, cb, vec = case
    p = rc.col_dot_problem(n + w, n, w, ld_a=ld_a - ca, ld_b=ld_b - cb, a_col=ca, b_col=cb, device=DEV)
    a, b = p["a"], p["b"]
    assert (a.ld, b.ld) == (ld_a, ld_b) and ld_a != ld_b and min(ld_a, ld_b) > w
    assert rc.col_dot_vector_path(w, a.ld, a.ptr, b.ld, b.ptr) == vec
    blocks, passes = rc.col_dot_shape(n, w)
    assert len(blocks) == (n + 511) // 512 and len(passes) == (w + 255) // 256
    for form in ("ordered", "atomic", "ops"):
        for which in ("ab", "s", "both"):
            o1, o2 = _col_dot_run(form, p, which)
            what = f"col_dot n={n} w={w} {form} {which}"
            rc.assert_exact(o1, rc.col_dot_expected(p, "want_a" if which == "s" else "want_ab", 2), what, p["span"])
            if o2 is not None:
                rc.assert_exact(o2, rc.col_dot_expected(p, "want_a", 2), what + " out_a", p["span"])


def test_the_case_tables_of_col_dot_hold_what_they_are_meant_to():
    assert {c[1] for c in COLDOT} == {1, 3, 4, 5, 20, 64, 128, 252, 256, 260, 516}
    assert {c[0] for c in COLDOT} == {1, 255, 256, 257, 511, 512, 513, 4 * 512 + 1, 9 * 512 - 1}
    scalar_mult4 = [c for c in COLDOT if c[1] % 4 == 0 and not c[6]]
    assert any(c[4] % 4 for c in scalar_mult4) and any(c[2] % 4 for c in scalar_mult4)
    groups = {rc.col_dot_shape(1, c[1])[1][0]["groups"] for c in COLDOT if c[6]}
    assert {5, 63} <= groups                                   # group counts that are no power of two, on 16-byte loads


def test_col_dot_through_ops_with_a_stale_cached_workspace():
    """ops keeps one workspace per stream: a large shape first, then a small one that reuses it with the large call's
    partials still inside.  Both equal a fresh C call with its own NaN workspace."""
    big = rc.col_dot_problem(1, 9 * 512 - 1, 256, ld_a=260, ld_b=264, device=DEV, calls=1)
    small = rc.col_dot_problem(2, 257, 5, ld_a=9, ld_b=8, device=DEV, calls=1)
    lib = _lib.load()
    ops._COLDOT_WORKSPACE.clear()
    for p in (big, small):
        got_ab, got_a = p["out0"].clone(), p["out0"].clone()
        ops.col_dot2(p["a"].full, p["a"].ld, p["b"].full, p["b"].ld, p["n"], p["width"], got_ab[p["span"]], got_a[p["span"]])
        ws, floats = rc.guarded_workspace(lib.cgnn_col_dot_workspace_bytes(p["n"], p["width"]), DEV)
        c_ab, c_a = p["out0"].clone(), p["out0"].clone()
        assert lib.cgnn_col_dot_ordered(p["a"].ptr, p["a"].ld, p["b"].ptr, p["b"].ld, p["n"], p["width"], c_ab[p["span"]].data_ptr(),
                                        c_a[p["span"]].data_ptr(), ws.data_ptr(), 4 * floats, _stream()) == 0
        torch.cuda.synchronize()
        rc.assert_guard(ws, floats, "col_dot fresh")
        rc.assert_exact(got_ab, c_ab, "ops against a fresh call, out_ab", p["span"])
        rc.assert_exact(got_a, c_a, "ops against a fresh call, out_a", p["span"])
        rc.assert_exact(c_ab, rc.col_dot_expected(p, "want_ab", 1), "fresh out_ab", p["span"])
        rc.assert_exact(c_a, rc.col_dot_expected(p, "want_a", 1), "fresh out_a", p["span"])
    (ws,) = ops._COLDOT_WORKSPACE.values()
    assert ws.numel() == lib.cgnn_col_dot_workspace_bytes(big["n"], big["width"])          # the small call did reuse it


# graphs of these many rows: boundaries at rows 2047, 2048 and 2049, empty graphs at the front, in the middle and at the end,
# one graph over three 2048-row blocks (one of them whole), a block that holds the ends of four graphs
SEGMENTS = [0, 2047, 1, 1, 0, 4100, 500, 600, 37, 0]


def _colsum_run(p, use_batch=True):
    lib = _lib.load()
    sums = p["sums0"].clone()
    batch = p["batch"] if use_batch else None
    code = lib.cgnn_segment_colsum(p["acc"].ptr, None if batch is None else batch.data_ptr(), p["n"], p["width"], p["num_graphs"],
                                   sums.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert code == 0, lib.cgnn_last_error()
    return sums


@pytest.mark.parametrize("width", [1, 3])
def test_segment_colsum_is_exact_at_graph_and_block_boundaries(width):
    p = rc.colsum_problem(width, SEGMENTS, width, DEV)
    ends = torch.tensor(SEGMENTS).cumsum(0).tolist()
    assert {2047, 2048, 2049} <= set(ends) and SEGMENTS[0] == SEGMENTS[4] == SEGMENTS[-1] == 0
    blocks = rc.colsum_blocks(p["n"])
    owners = [sorted({int(x) for x in p["batch"][r0:r1].unique()}) for r0, r1 in blocks]
    assert sum(1 for o in owners if 5 in o) == 3 and [5] in owners and max(len(o) for o in owners) >= 3
    assert p["acc"].ld == width                                    # contiguous rows: the entry takes no leading dimension
    rc.assert_exact(_colsum_run(p), p["want"], f"segment_colsum width {width}", (slice(0, p["num_graphs"]),))
    got = ops.segment_colsum(p["acc"].values, p["batch"][:p["n"]], p["num_graphs"])
    assert torch.equal(got, p["want"][:-1])
    for n in (2049, p["n"]):                                         # batch NULL: one graph, two and four blocks
        q = rc.colsum_problem(n, None, (n, width), DEV)
        rc.assert_exact(_colsum_run(q, False), q["want"], f"segment_colsum batch NULL n={n}", (slice(0, 1),))
        assert torch.equal(ops.segment_colsum(q["acc"].values, None, 1), q["want"][:-1])


# ---- arithmetic, per element, at 64 rows ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real(out_dim, in_dim):
    return rc.model_problem(out_dim, in_dim)


@functools.lru_cache(maxsize=None)
def _db_yard():
    return rc.pooled_db_yardstick()


@pytest.mark.parametrize("shape", rc.MODEL_LINEARS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rounding_per_element_is_that_of_a_float32_product(shape):
    """Real inputs with full mantissas, a column block x 1e-3 and a row block x 1e-8: EVERY element of dw (db) within 4 x what
    torch's float32 product on the CPU loses on the same problem, measured against its own sum of absolute terms (db: within
    4 x the yardstick's worst over the column sums of all six shapes, reduction_checks.pooled_db_yardstick)."""
    o, i = shape
    p = _real(o, i)
    lib = _lib.load()
    g, a = p["g"].to(DEV), p["a"].to(DEV)
    n = p["n"]
    forms = ["ordered", "atomic", "ops"] + (["x3", "ops_x3"] if shape == (128, 128) else [])
    worst = {}
    for form in forms:
        dw, db = torch.zeros(o, i, device=DEV), torch.zeros(o, device=DEV)
        if form == "ordered":
            ws, floats = rc.guarded_workspace(lib.cgnn_weight_grad_workspace_bytes(n, o, i), DEV)
            code = lib.cgnn_weight_grad_ordered(g.data_ptr(), o, o, a.data_ptr(), i, i, n, dw.data_ptr(), i, 0, db.data_ptr(),
                                                ws.data_ptr(), 4 * floats, _stream())
        elif form == "atomic":
            code = lib.cgnn_weight_grad(g.data_ptr(), o, o, a.data_ptr(), i, i, n, dw.data_ptr(), i, 0, db.data_ptr(), _stream())
        elif form == "x3":
            ws, floats = rc.guarded_workspace(lib.cgnn_weight_grad_x3_workspace_bytes(), DEV)
            code = lib.cgnn_weight_grad_x3(g.data_ptr(), o, a.data_ptr(), i, n, dw.data_ptr(), i, 0, db.data_ptr(), ws.data_ptr(),
                                           4 * floats, _stream())
        else:
            ops.weight_grad(g, o, o, a, i, n, dw, 0, db, "fp32x3" if form == "ops_x3" else "fp32")
            code = 0
        assert code == 0, (form, lib.cgnn_last_error())
        torch.cuda.synchronize()
        worst[form] = (rc.elem_ratio(dw, p["want"], p["S"]), rc.elem_ratio(db, p["want_b"], p["S_b"]))
    print(f"reduction-gate {o}x{i} n={n}: float32 yardstick dw {p['yard']:.2e} db {p['yard_b']:.2e} (pooled {_db_yard():.2e}) | " +
          " | ".join(f"{f} dw {w:.2e} db {b:.2e}" for f, (w, b) in worst.items()))
    for form, (w, b) in worst.items():
        assert w <= rc.ARITH_MARGIN * p["yard"], (form, "dw", w, p["yard"])
        assert b <= rc.ARITH_MARGIN * _db_yard(), (form, "db", b, _db_yard())
