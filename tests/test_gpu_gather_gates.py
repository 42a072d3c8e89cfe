"""GPU: the kernels that only move rows or sum them by index, gated EXACTLY (tests/gather_checks.py; the gates are tested on
themselves in tests/test_gather_gates_cpu.py): cgnn_aggregate in its four forms, cgnn_csr_build with the shared scan,
cgnn_aggregate_csr_add, cgnn_halo_return_add, cgnn_gather_rows / cgnn_scatter_rows and cgnn_relayout.  Tables hold small
integers, so the float atomics' arrival order, the pairwise tree and the sequential loops all have to give the bits of an
int64 ``index_add_`` on the CPU; tables lie between NaN rows (a row read from outside fails), outputs inside a pattern of
canaries that is compared bit for bit.  The sizes come from the finders for this device's compute units; each test asserts
from the restated geometry that the branch it is named for is entered.  The documented summation orders are probed with
2^24, 1, 1, -2^24, whose float32 sum is 0 in ascending order, 2 in reverse and 1 pairwise.

Left out: the ``1 << 20``-workgroup clamp of cgnn_aggregate_csr_add and cgnn_halo_return_add needs 2^28 work items (a table
of more than 4 GiB at width 4), and the plain stride of xcd_work_range cannot be reached through cgnn_aggregate, whose grid is
a multiple of 8 for every total (pinned on the CPU)."""
import functools

import pytest
import torch

import gather_checks as gc
import reduction_checks as rc
from cosmology_gnn_simulation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = rc.PAD_ROWS


@functools.lru_cache(None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _block(padded):
    """The block of a Padded tensor on the device as the contiguous view the kernels get."""
    v = padded.full[padded.block]
    assert v.is_contiguous() and (v.numel() == 0 or v.data_ptr() == padded.full.data_ptr() + 4 * PAD * padded.width)
    return v


# ---- cgnn_aggregate --------------------------------------------------------------------------------------------------------
def _aggregate_check(p, fixed_k, what):
    table, out = p["table"].to(DEV), p["out"].to(DEV)
    tb = ops.TiledRows(p["table_rows"], p["width"], DEV, buf=_block(table)) if p["tiled"] else _block(table)
    gather = None if p["gather"] is None else p["gather"].to(DEV)
    dst = p["dst"].to(DEV) if fixed_k == 0 else None
    got = ops.aggregate(tb, gather, dst, p["num_nodes"], fixed_k, p["num_edges"], _block(out))
    assert got.data_ptr() == _block(out).data_ptr()
    rc.assert_exact(out.full.cpu(), p["out"].expected(p["want"]), what, p["out"].block)


@pytest.mark.parametrize("width", gc.FIXEDK_WIDTHS)
@pytest.mark.parametrize("k", gc.FIXEDK_KS)
def test_fixed_k_rows_is_exact_on_every_eighth(k, width):
    """aggregate_fixedk_kernel: 8 workgroups with an empty eighth, and more than 8 with total % 2048 != 0 (total % 8 != 0 at
    widths 4 and 36); ``gather`` with repeated senders and ``gather == NULL`` (row e0 + j)."""
    sizes = gc.fixedk_sizes(width, _cus())
    for name, n in sizes.items():
        total, nb = gc.grid_for("fixedk_rows", n, width, _cus())
        assert nb % 8 == 0 and (nb == 8) == (name == "one_block_per_eighth") and gc.passes(total, nb, True) == 1
        assert name != "ragged_eighths" or (total % 2048 != 0 and (total % 8 != 0) == (width in (4, 36)))
        for senders in ("random", None):
            p = gc.aggregate_problem(1000 * k + n, n, width, gc.fixedk_dst(n, k), senders=senders, table_rows=n + 3)
            _aggregate_check(p, k, f"fixed k {k} width {width} {name} {senders}")


@pytest.mark.parametrize("k", (8, 3), ids=("tree", "generic"))
def test_fixed_k_rows_second_trip_through_the_grid(k):
    n = gc.first_second_pass("fixedk_rows", 256, _cus())
    total, nb = gc.grid_for("fixedk_rows", n, 256, _cus())
    assert nb == _cus() * gc.CAP_FIXEDK // 8 * 8 and gc.passes(total, nb, True) == 2 and gc.passes(total - 64, nb, True) == 1
    p = gc.aggregate_problem(k, n, 256, gc.fixedk_dst(n, k), senders="random")
    _aggregate_check(p, k, f"second trip, n = {n}")


@pytest.mark.parametrize("width", gc.TILED_WIDTHS)
@pytest.mark.parametrize("k", gc.TILED_KS)
def test_fixed_k_tiled_messages_are_exact(k, width):
    """aggregate_fixedk_tiled_kernel on a TILED32 buffer laid out by ``tiled_offsets`` on the CPU; n k is no multiple of 32 and
    the pad rows of the last tile are NaN."""
    for n in (1, 45, 1027):
        assert (n * k) % 32 != 0
        p = gc.aggregate_problem(k * n, n, width, gc.fixedk_dst(n, k), tiled=True)
        _aggregate_check(p, k, f"tiled k {k} width {width} n {n}")


def test_fixed_k_tiled_second_trip_through_the_grid():
    n = gc.first_second_pass("fixedk_tiled", 256, _cus())
    total, nb = gc.grid_for("fixedk_tiled", n, 256, _cus())
    assert nb == _cus() * gc.CAP_FIXEDK and gc.passes(total, nb) == 2 and gc.passes(total - 64, nb) == 1
    _aggregate_check(gc.aggregate_problem(2, n, 256, gc.fixedk_dst(n, 2), tiled=True), 2, f"tiled second trip, n = {n}")


@pytest.mark.parametrize("width", (4, 256))
@pytest.mark.parametrize("k", (4, 5, 8, 16, 17))
def test_fixed_k_summation_order(k, width):
    """Ascending j in the generic loop, the pairwise tree at k = 8 / 16: through ``gather`` and on TILED32 messages."""
    a = gc.probe_addends(k)
    f = gc.column_factors(width)
    want = gc.documented_sum(a)[:, None] * f[None, :]
    n = a.shape[0]
    table = gc.Padded(gc.PROBE_TABLE[:, None] * f[None, :]).to(DEV)
    out = gc.Padded(shape=(n, width), fill="pattern").to(DEV)
    ops.aggregate(_block(table), gc.probe_gather(a).to(DEV), None, n, k, n * k, _block(out))
    rc.assert_exact(out.full.cpu(), gc.Padded(shape=(n, width), fill="pattern").expected(want), f"order k {k}", out.block)
    if width % 32 == 0:
        msg = a.reshape(-1, 1) * f[None, :]
        tiled = gc.Padded(gc.to_tiled(msg, rc.NAN).view(-1, width)).to(DEV)
        out = gc.Padded(shape=(n, width), fill="pattern").to(DEV)
        ops.aggregate(ops.TiledRows(n * k, width, DEV, buf=_block(tiled)), None, None, n, k, n * k, _block(out))
        rc.assert_exact(out.full.cpu(), gc.Padded(shape=(n, width), fill="pattern").expected(want), f"tiled order k {k}", out.block)


FORMS = ("gather", "edge", "tiled")


@pytest.mark.parametrize("width,form", [(w, f) for w in gc.GENERAL_WIDTHS for f in FORMS if f != "tiled" or w % 32 == 0])
def test_general_list_is_exact_at_every_group_wave_and_block_edge(width, form):
    """aggregate_scatter_kernel (widths 32 ... 256) and aggregate_atomic_kernel (4, 36): every edge list at every edge count,
    through ``gather``, by edge id and (widths that TILED32 takes) on TILED32 messages."""
    geo = gc.general_geometry(width, 1)
    for cname, e in gc.edge_counts(width).items():
        g = gc.general_geometry(width, e)
        assert g["blocks"] >= 2 and e >= geo["block_edges"] + geo["wave_edges"] - 1
        for lname in gc.EDGE_LISTS:
            dst, n = gc.edge_list(lname, e, width)
            p = gc.aggregate_problem(e, n, width, dst, senders="random" if form == "gather" else None, table_rows=n + 3,
                                     tiled=form == "tiled")
            _aggregate_check(p, 0, f"width {width} {form} {cname} {lname}")


@pytest.mark.parametrize("width", gc.GENERAL_WIDTHS)
def test_general_list_hub_and_tiny_lists(width):
    dst, n = gc.edge_list("one_destination", 1 << 12, width)                   # 2^12 edges into one row
    _aggregate_check(gc.aggregate_problem(5, n, width, dst, senders="random", table_rows=64), 0, "2^12 edges into one row")
    mixed = torch.cat([torch.arange(100), torch.full((1 << 12,), 50), torch.arange(100, 177)])
    _aggregate_check(gc.aggregate_problem(6, 177, width, mixed, senders="random", table_rows=64), 0, "a hub inside a list")
    for e in (0, 1):
        for tiled in ((False, True) if width % 32 == 0 and e else (False,)):
            p = gc.aggregate_problem(e, 3, width, torch.full((e,), 2, dtype=torch.int64), tiled=tiled,
                                     senders=None if e else "random", table_rows=5)       # no edges: still a table to name
            _aggregate_check(p, 0, f"{e} edges")


# ---- cgnn_csr_build ----------------------------------------------------------------------------------------------------------
def _csr_build(key, val, rows):
    """One cgnn_csr_build into guarded buffers -> (row_ptr, col) on the CPU; the workspace is NaN bytes with a guard behind
    the reported size, row_ptr and col lie inside sentinels."""
    lib = _lib.load()
    e = key.numel()
    nbytes = lib.cgnn_csr_workspace_bytes(rows)
    assert nbytes == gc.csr_workspace_bytes(rows)
    ws, floats = rc.guarded_workspace(nbytes, DEV)
    ws[:floats].view(torch.uint8).fill_(255)
    rp_full = torch.full((rows + 1 + 32,), -77, dtype=torch.int32, device=DEV)
    col_full = torch.full((e + 80,), -99, dtype=torch.int32, device=DEV)
    rp, col = rp_full[16:16 + rows + 1], col_full[16:16 + e]
    kd = key.to(DEV)
    vd = None if val is None else val.to(DEV)
    code = lib.cgnn_csr_build(kd.data_ptr() if e else None, None if vd is None or not e else vd.data_ptr(), e, rows, rp.data_ptr(),
                              col_full.data_ptr() + 64, ws.data_ptr(), nbytes, _stream())
    assert code == 0, lib.cgnn_last_error()
    torch.cuda.synchronize()
    rc.assert_guard(ws, floats, "cgnn_csr_build")
    assert bool((rp_full[:16] == -77).all()) and bool((rp_full[16 + rows + 1:] == -77).all()), "row_ptr's neighbours"
    assert bool((col_full[:16] == -99).all()) and bool((col_full[16 + e:] == -99).all()), "col beyond e"
    return rp.cpu(), col.cpu()


@functools.lru_cache(None)
def _csr_case(rows, last):
    return gc.csr_keys(rows, rows, last)


@pytest.mark.parametrize("rows,last", gc.csr_rows_cases())
def test_csr_build_is_exact(rows, last):
    k = _csr_case(rows, last)
    assert gc.scan_blocks(rows + 1) == (rows + 1 + 2047) // 2048
    for val in (k["val"], None):
        want_ptr, want_col = gc.csr_reference(k["key"], val, rows)
        got_ptr, got_col = _csr_build(k["key"], val, rows)
        assert torch.equal(got_ptr, want_ptr), "row_ptr"
        assert torch.equal(got_col, want_col), "col"
        again = ops.SenderCsr(k["key"].to(DEV), None if val is None else val.to(DEV), rows)
        assert torch.equal(again.row_ptr.cpu(), got_ptr) and torch.equal(again.col.cpu()[:k["key"].numel()], got_col)


def test_csr_build_refuses_keys_outside_its_rows():
    for bad in (4, -1):                                          # key == num_rows, key == -1, not at the first position
        src = torch.tensor([0, 3, bad, 1], dtype=torch.int32, device=DEV)
        with pytest.raises(ops.CgnnError, match="outside"):
            ops.SenderCsr(src, torch.zeros_like(src), 4)
    src = torch.tensor([0, 5, 1], dtype=torch.int32, device=DEV)
    with pytest.raises(ops.CgnnError, match="outside"):
        ops.SenderCsr(src, src, 4)


# ---- cgnn_aggregate_csr_add ------------------------------------------------------------------------------------------------
ADDENDS = ("none", "add1", "add2", "both", "out_is_add1", "out_is_add2")


def _csr_add_check(csr, table, want_sum, a, b, mode, width, seed, what):
    gen = torch.Generator().manual_seed(seed)
    v1, v2 = rc.int_matrix(gen, b - a, width, "cpu"), rc.int_matrix(gen, b - a, width, "cpu")
    use1, use2 = mode in ("add1", "both", "out_is_add1", "out_is_add2"), mode in ("add2", "both", "out_is_add1", "out_is_add2")
    want = want_sum[a:b] + (v1 if use1 else 0) + (v2 if use2 else 0)
    host = gc.Padded({"out_is_add1": v1, "out_is_add2": v2}.get(mode), shape=(b - a, width), fill="pattern")
    out = host.to(DEV)
    ob = _block(out)
    add1 = ob if mode == "out_is_add1" else (v1.to(DEV) if use1 else None)
    add2 = ob if mode == "out_is_add2" else (v2.to(DEV) if use2 else None)
    got = ops.aggregate_csr(table, csr, out=ob, add1=add1, add2=add2, row_range=None if (a, b) == (0, csr.rows) else (a, b))
    assert got is ob
    rc.assert_exact(out.full.cpu(), host.expected(want), f"{what} rows [{a}, {b}) {mode}", host.block)


@pytest.mark.parametrize("rows,last", gc.csr_rows_cases())
def test_aggregate_csr_add_is_exact(rows, last):
    """Every addend / alias combination on the whole CSR, and row ranges (a, b), (a, a), (rows - 1, rows) with the combinations
    taken in turn; the planted rows hold every remainder of the four-way unroll."""
    k = _csr_case(rows, last)
    csr = ops.SenderCsr(k["key"].to(DEV), k["val"].to(DEV), rows)
    row_ptr, col = gc.csr_reference(k["key"], k["val"], rows)
    lengths = (row_ptr[1:] - row_ptr[:-1])
    assert rows < 58 or {0, 1, 2, 3} <= set((lengths % 4).tolist())
    ranges = [r for r in ((rows // 3 + 1, 2 * rows // 3 + 2), (rows // 2, rows // 2), (rows - 1, rows)) if 0 <= r[0] <= r[1] <= rows
              and (r[0] > 0 or rows <= 1)]
    for width in gc.CSR_ADD_WIDTHS:
        host = gc.Padded(rc.int_matrix(torch.Generator().manual_seed(width), k["table_rows"], width, "cpu"))
        table = _block(host.to(DEV))
        want_sum = gc.segment_sum_reference(host.values, row_ptr, col, 0, rows)
        for i, mode in enumerate(ADDENDS):
            _csr_add_check(csr, table, want_sum, 0, rows, mode, width, i, f"width {width}")
        for j, (a, b) in enumerate(ranges):
            for i in (j, j + 3):
                _csr_add_check(csr, table, want_sum, a, b, ADDENDS[(i + width // 4) % 6], width, 10 + i, f"width {width}")
    if rows > 3:
        assert any(0 < a < b < rows for a, b in ranges) and any(a == b for a, b in ranges) and (rows - 1, rows) in ranges


@pytest.mark.parametrize("width", (4, 128))
def test_aggregate_csr_summation_order(width):
    """Ascending p inside a row (the CSR's rows are sorted by value, so table rows 4 i ... 4 i + 3 are taken in that order), then
    (add1 + add2) + sum."""
    a = gc.probe_addends(4)
    f = gc.column_factors(width)
    r = a.shape[0]
    key = torch.arange(r, dtype=torch.int32).repeat_interleave(4)
    val = torch.arange(4 * r, dtype=torch.int32)
    shuffle = torch.randperm(4 * r, generator=torch.Generator().manual_seed(1))
    csr = ops.SenderCsr(key[shuffle].to(DEV), val[shuffle].to(DEV), r)
    table = gc.Padded(a.reshape(-1, 1) * f[None, :]).to(DEV)
    got = ops.aggregate_csr(_block(table), csr)
    rc.assert_exact(got.cpu(), gc.sequential_sum(a)[:, None] * f[None, :], "ascending p")
    # one edge of 2^24 per row, add1 = add2 = 1: (1 + 1) + 2^24 = 2^24 + 2; 1 + (1 + 2^24) and (2^24 + 1) + 1 give 2^24
    csr1 = ops.SenderCsr(torch.arange(r, dtype=torch.int32, device=DEV), torch.zeros(r, dtype=torch.int32, device=DEV), r)
    big = gc.Padded(torch.full((1, width), gc.BIG)).to(DEV)
    ones = torch.ones(r, width, device=DEV)
    got = ops.aggregate_csr(_block(big), csr1, add1=ones, add2=ones.clone())
    rc.assert_exact(got.cpu(), torch.full((r, width), gc.BIG + 2), "(add1 + add2) + sum")


# ---- cgnn_halo_return_add ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", gc.HALO_WIDTHS)
def test_halo_return_add_is_exact_and_accumulates(width):
    gen = torch.Generator().manual_seed(width)
    t_rows, r_rows = 64, 40
    host = gc.Padded(rc.int_matrix(gen, t_rows, width, "cpu"), fill="pattern")
    ret_host = gc.Padded(rc.int_matrix(gen, r_rows, width, "cpu"))
    rows, seg_ptr, col = gc.halo_plan(width, t_rows, r_rows)
    assert sorted(set((seg_ptr[1:] - seg_ptr[:-1]).tolist())) == list(range(10))
    add = gc.segment_sum_reference(ret_host.values, seg_ptr, col, 0, rows.numel())
    table, ret = host.to(DEV), ret_host.to(DEV)
    want = host.values.clone()
    for call in (1, 2):
        ops.halo_return_add(_block(table), _block(ret), rows.to(DEV), seg_ptr.to(DEV), col.to(DEV))
        want[rows.long()] += add
        rc.assert_exact(table.full.cpu(), host.expected(want), f"width {width} call {call}", host.block)    # unnamed rows too


@pytest.mark.parametrize("width", (4, 256))
def test_halo_return_add_summation_order(width):
    """The table's own row first, then ascending p: 2^24 in the table, 1, 1, -2^24 returned (and the permutations)."""
    a = gc.probe_addends(4)
    f = gc.column_factors(width)
    r = a.shape[0]
    host = gc.Padded(a[:, :1] * f[None, :], fill="pattern")
    ret = gc.Padded(a[:, 1:].reshape(-1, 1) * f[None, :]).to(DEV)
    table = host.to(DEV)
    rows = torch.arange(r, dtype=torch.int32, device=DEV)
    seg_ptr = torch.arange(0, 3 * r + 1, 3, dtype=torch.int32, device=DEV)
    col = torch.arange(3 * r, dtype=torch.int32, device=DEV)
    ops.halo_return_add(_block(table), _block(ret), rows, seg_ptr, col)
    want = gc.sequential_sum(a[:, 1:], a[:, 0])[:, None] * f[None, :]
    assert torch.equal(want[:, 0], gc.sequential_sum(a)) and float(want[0, 0]) == 0.0
    rc.assert_exact(table.full.cpu(), host.expected(want), "own row first", host.block)


def test_halo_return_add_skips_rows_and_positions_outside_the_tables():
    """The documented guard, inside allocations that keep even a broken guard in owned memory: rows -1 and table_rows are
    skipped with their segments, a position ret_rows adds nothing.  Nothing changes."""
    width, t_rows, r_rows = 128, 40, 24
    gen = torch.Generator().manual_seed(3)
    host = gc.Padded(rc.int_matrix(gen, t_rows, width, "cpu"), fill="pattern")
    ret_host = gc.Padded(rc.int_matrix(gen, r_rows, width, "cpu"), fill=5.0)
    table, ret = host.to(DEV), ret_host.to(DEV)
    rows = torch.tensor([-1, t_rows, 7], dtype=torch.int32, device=DEV)
    seg_ptr = torch.tensor([0, 3, 8, 9], dtype=torch.int32, device=DEV)
    col = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, r_rows], dtype=torch.int32, device=DEV)
    ops.halo_return_add(_block(table), _block(ret), rows, seg_ptr, col)
    rc.assert_exact(table.full.cpu(), host.full, "guarded plan", slice(0, 0))
    rc.assert_exact(ret.full.cpu(), ret_host.full, "ret", slice(0, 0))


# ---- cgnn_gather_rows / cgnn_scatter_rows ------------------------------------------------------------------------------------
def _rows_check(n_idx, width, what):
    p = gc.rows_problem(n_idx + width, n_idx, width)
    table, out = p["table"].to(DEV), p["out"].to(DEV)
    idx = p["idx_full"].to(DEV)[:n_idx]
    ops.gather_rows(_block(table), idx, _block(out))
    rc.assert_exact(out.full.cpu(), p["out"].expected(p["gathered"]), f"gather {what}", p["out"].block)
    assert torch.equal(ops.gather_rows(_block(table), idx).cpu(), p["gathered"])
    rows, dest = p["rows"].to(DEV), p["dest"].to(DEV)
    ops.scatter_rows(_block(rows), p["perm_full"].to(DEV)[:n_idx], _block(dest))
    want = p["dest"].values.clone().index_copy_(0, p["perm"].long(), p["rows"].values)       # the whole table: untouched rows too
    rc.assert_exact(dest.full.cpu(), p["dest"].expected(want), f"scatter {what}", p["dest"].block)


@pytest.mark.parametrize("width", gc.ROWS_WIDTHS)
def test_gather_and_scatter_rows_are_exact(width):
    """Widths that are no multiple of 4 take the scalar kernels; duplicates in the gather, a permutation subset in the scatter;
    the lists are slices of longer ones whose tail would move a NaN row."""
    for n_idx in gc.ROWS_N_IDX:
        _rows_check(n_idx, width, f"width {width} n_idx {n_idx}")


def test_empty_index_lists_and_row_ranges_move_nothing():
    """An empty tensor has no address: the wrappers return before the library refuses a NULL pointer."""
    _rows_check(0, 36, "no index")
    csr = ops.SenderCsr(torch.tensor([1, 1, 0], dtype=torch.int32, device=DEV), None, 3)
    table = torch.ones(3, 8, device=DEV)
    assert ops.aggregate_csr(table, csr, row_range=(2, 2)).shape == (0, 8)
    assert torch.equal(ops.aggregate_csr(table, csr).cpu(), torch.tensor([1.0, 2.0, 0.0])[:, None].expand(3, 8))


def test_gather_and_scatter_rows_second_trip_through_the_grid():
    for kind in ("gather_rows", "scatter_rows"):
        n = gc.first_second_pass(kind, 256, _cus())
        total, nb = gc.grid_for(kind, n, 256, _cus())
        assert nb == _cus() * gc.CAP_ROWS and gc.passes(total, nb) == 2 and gc.passes(total - 64, nb) == 1
    _rows_check(n, 256, f"second trip, n_idx = {n}")


# ---- cgnn_relayout ---------------------------------------------------------------------------------------------------------
def _relayout_check(n, width):
    lib = _lib.load()
    x = rc.int_matrix(torch.Generator().manual_seed(n + width), n, width, "cpu")
    rows_src = gc.Padded(x).to(DEV)
    tiled_src = gc.Padded(gc.to_tiled(x, rc.NAN).view(-1, width)).to(DEV)
    tiled_want, n_pad = gc.to_tiled(x, 0.0), gc.tiled_rows(n)
    for src, frm, to, want in ((rows_src, _lib.ROWS, _lib.TILED32, tiled_want), (tiled_src, _lib.TILED32, _lib.ROWS, x.reshape(-1)),
                               (tiled_src, _lib.TILED32, _lib.TILED32, tiled_want), (rows_src, _lib.ROWS, _lib.ROWS, x.reshape(-1))):
        dst = torch.full(((n_pad + 2 * PAD) * width,), rc.NAN, device=DEV)           # NaN before, behind and on the pad rows
        want_full = torch.full(((n_pad + 2 * PAD) * width,), rc.NAN)
        want_full[PAD * width:PAD * width + want.numel()] = want
        code = lib.cgnn_relayout(_block(src).data_ptr(), frm, dst.data_ptr() + 4 * PAD * width, to, n, width, _stream())
        assert code == 0, lib.cgnn_last_error()
        rc.assert_exact(dst.cpu(), want_full, f"relayout n {n} width {width} {frm} -> {to}", slice(0, 0))
        if to == _lib.TILED32 and n_pad > n:
            pads = dst.cpu()[PAD * width:][gc.tiled_offsets(n_pad, width, first_row=n).reshape(-1)]
            assert bool((pads.view(torch.int32) == 0).all()), "the pad rows are +0.0"
    # the wrappers: rows -> TiledRows, and TiledRows -> the first n rows of a longer out
    t = ops.TiledRows.from_rows(_block(rows_src))
    mask = torch.ones(n_pad * width, dtype=torch.bool)
    mask[gc.tiled_offsets(n, width).reshape(-1)] = False
    got = t.buf.cpu().view(-1)
    assert torch.equal(got[~mask], tiled_want[~mask]) and bool((got[mask].view(torch.int32) == 0).all())
    host = gc.Padded(shape=(n + 5, width), fill="pattern")
    out = host.to(DEV)
    ops.relayout(ops.TiledRows(n, width, DEV, buf=_block(tiled_src)), out=_block(out))
    want = host.values.clone()
    want[:n] = x
    rc.assert_exact(out.full.cpu(), host.expected(want), f"relayout into a longer out, n {n}", host.block)


@pytest.mark.parametrize("width", gc.RELAYOUT_WIDTHS)
@pytest.mark.parametrize("n", gc.RELAYOUT_N)
def test_relayout_moves_every_element_and_zeroes_the_pad_rows(n, width):
    _relayout_check(n, width)


def test_relayout_second_trip_through_the_grid():
    n = gc.first_second_pass("relayout", 256, _cus())
    total, nb = gc.grid_for("relayout", gc.tiled_rows(n), 256, _cus())
    assert nb == _cus() * gc.CAP_ROWS and gc.passes(total, nb) == 2 and n % 32 == 1
    _relayout_check(n, 256)


# ---- wrapper refusals --------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_shapes_that_would_leave_a_tensor():
    """Each of these made a kernel read or write past a tensor; now nothing is launched (the destinations keep their bits)."""
    gen = torch.Generator().manual_seed(0)
    table = rc.int_matrix(gen, 20, 8, "cpu").to(DEV)
    idx = torch.tensor([3, 1, 4, 1, 5], dtype=torch.int32, device=DEV)
    canary = gc.pattern(20, 8, DEV)
    dest = canary.clone()
    for rows in (torch.zeros(4, 8, device=DEV), torch.zeros(5, 4, device=DEV), torch.zeros(40, device=DEV)):
        with pytest.raises(ops.CgnnError, match="scatter_rows"):
            ops.scatter_rows(rows, idx, dest)
    for out in (dest[:4], dest[:5, :4], dest[:6], dest[:5].double()):
        with pytest.raises(ops.CgnnError, match="gather_rows"):
            ops.gather_rows(table, idx, out)
    dst = torch.tensor([0, 0, 1, 2, 2], dtype=torch.int32, device=DEV)
    for out in (dest[:2], dest[:3, :4], dest[:4], dest[:3].double()):
        with pytest.raises(ops.CgnnError, match="aggregate: out"):
            ops.aggregate(table, idx, dst, 3, 0, 5, out)
    with pytest.raises(ops.CgnnError, match="aggregate: a table of 4 rows"):
        ops.aggregate(table[:4], None, dst, 3, 0, 5, dest[:3])
    with pytest.raises(ops.CgnnError, match="aggregate: a table of 20 rows"):
        ops.aggregate(table, None, None, 7, 3, 21, dest[:7])
    torch.cuda.synchronize()
    assert torch.equal(dest.view(torch.int32), canary.view(torch.int32))
    # the valid calls next to them still run
    assert torch.equal(ops.gather_rows(table, idx, dest[:5]).cpu(), table.cpu()[idx.cpu().long()])
    perm = torch.tensor([3, 1, 4, 0, 5], dtype=torch.int32, device=DEV)
    want = dest.clone().index_copy_(0, perm.long(), table[:5])
    assert torch.equal(ops.scatter_rows(table[:5], perm, dest), want)
    got = ops.aggregate(table, idx, dst, 3, 0, 5, dest[:3]).cpu()
    assert torch.equal(got, torch.zeros(3, 8).index_add_(0, dst.cpu().long(), table.cpu()[idx.cpu().long()]))
