"""GPU: every compiled form of ``aggregate_planned_kernel`` (K in {8, 16, runtime} x SL in {4, 8, runtime}; which one a
call runs is asserted through ``cgnn_aggregate_planned_form``) at chosen block contents: sender lists from
tests/aggregate_plan_checks.py whose blocks hold 1 .. rows * k distinct senders on both sides of the staging limit (352)
and of the list's capacity (512).  Every sum is compared three ways: bit for bit with the CPU restatement of the kernel's
summation order, bit for bit with ``cgnn_aggregate`` without a plan, and with the float64 sum within k - 1 roundings.
The plan blob is read back and checked field by field.  Every index is in range and every buffer as large as the
contract says."""
import numpy as np
import pytest
import torch

import aggregate_plan_checks as apc
from cosmology_gnn_simulation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                      # guard rows before and after `out` and the table
SENTINEL = 0x7FA5A5A5           # a NaN no sum produces: a kernel that wrote a guard row cannot have restored it


def _form(table_rows, n, k, width):
    return _lib.load().cgnn_aggregate_planned_form(table_rows, n, k, width)


def _guarded(rows, width, fill=None):
    """A [rows, width] float32 view with GUARD rows before and after it: (whole buffer, view)."""
    buf = torch.empty(rows + 2 * GUARD, width, device=DEV)
    if fill is None:
        buf.view(torch.int32).fill_(SENTINEL)
    else:
        buf.fill_(fill)
    return buf, buf[GUARD: GUARD + rows]


def _guards_untouched(buf, rows):
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + rows:] == SENTINEL).all())


def _device_table(table):
    """The CPU table as a view inside a device buffer whose rows before and after it are NaN."""
    buf, view = _guarded(table.shape[0], table.shape[1], fill=float("nan"))
    view.copy_(table)
    return buf, view


def _run(table, src, plan, n, k, route, out):
    """The planned kernel through the C entries: "rows" with the table's row count, "norows" without."""
    lib, width = _lib.load(), table.shape[1]
    assert table.is_contiguous() and out.is_contiguous() and out.shape == (n, width)
    if route == "rows":
        rc = lib.cgnn_aggregate_planned_rows(table.data_ptr(), table.shape[0], src.data_ptr(), plan.blob.data_ptr(), n, k,
                                             width, out.data_ptr(), _lib.stream_ptr(table.device))
    else:
        rc = lib.cgnn_aggregate_planned(table.data_ptr(), src.data_ptr(), plan.blob.data_ptr(), n, k, width,
                                        out.data_ptr(), _lib.stream_ptr(table.device))
    _lib.check(rc, "cgnn_aggregate_planned")
    return out


def _planned(table, src, plan, n, k, route):
    """One guarded run: the output (CPU); the guard rows around it must be untouched."""
    buf, out = _guarded(n, table.shape[1])
    _run(table, src, plan, n, k, route, out)
    assert _guards_untouched(buf, n), "the kernel wrote outside its num_nodes rows"
    return out.cpu()


def _differing_rows(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    diff = (na != nb) | ((a.view(torch.int32) != b.view(torch.int32)) & ~na)
    return torch.nonzero(diff.any(dim=1)).flatten().tolist()[:12]


def _compare_three_ways(got, table_cpu, table_dev, src_cpu, src_dev, n, k, what=""):
    want = apc.sum_kernel_order(table_cpu, src_cpu, n, k)
    assert apc.same_bits(got, want), f"{what}: rows {_differing_rows(got, want)} differ from the kernel-order sum"
    plain = ops.aggregate(table_dev, src_dev, None, n, k).cpu()
    assert apc.same_bits(got, plain), f"{what}: rows {_differing_rows(got, plain)} differ from cgnn_aggregate"
    finite = torch.isfinite(table_cpu[src_cpu.long()].view(n, k, -1)).all(dim=1)
    exact, bound = apc.sum_f64(table_cpu, src_cpu, n, k), apc.sum_bound(table_cpu, src_cpu, n, k)
    err = (got.double() - exact).abs()
    worst = float((err[finite] / bound[finite].clamp_min(1e-300)).max()) if k > 1 else 0.0
    print(f"{what}: largest error / bound = {worst:.3f}")
    assert bool((err[finite] <= bound[finite]).all()), f"{what}: beyond (k - 1) 2^-24 sum |x| of the float64 sum"
    return want


def _table(rows, width, seed):
    return torch.randn(rows, width, generator=torch.Generator().manual_seed(seed))


def _ids(case):
    return f"k{case[0]}-w{case[1]}-{case[2]}-form{case[3]}"


@pytest.mark.parametrize("case", apc.FORM_CASES, ids=_ids)
def test_every_form_at_every_block_content(case):
    """U = 1, 2, 31, 32, 33, 351, 352, 353, 511, 512, 513 and rows * k distinct senders per block (what rows * k allows),
    twice each in shuffled order, then a partial block; senders reach row 0 and the last ghost row; `out` and the table
    sit between guard rows."""
    k, width, route, form = case
    src_cpu, blocks, n, table_rows = apc.form_case_senders(k, seed=k)
    assert _form(table_rows if route == "rows" else 0, n, k, width) == form
    assert int(src_cpu.max()) == table_rows - 1 and int(src_cpu.min()) == 0
    src = src_cpu.to(DEV)
    plan = ops.AggregatePlan(src, n, k)
    apc.check_plan(plan.blob.cpu(), src_cpu, n, k)
    table_cpu = _table(table_rows, width, seed=1000 + k + width)
    _, table = _device_table(table_cpu)
    got = _planned(table, src, plan, n, k, route)
    assert bool(torch.isfinite(got).all()), "a finite table gave a non-finite sum: rows outside the table were read"
    _compare_three_ways(got, table_cpu, table, src_cpu, src, n, k, _ids(case))
    again = _planned(table, src, plan, n, k, route)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


def _grid_ids(p):
    return f"k{p[0]}-w{p[1]}"


@pytest.mark.parametrize("k,width", apc.GRID_FORMS, ids=[_grid_ids(p) for p in apc.GRID_FORMS])
def test_partial_last_block_and_grid_shapes(k, width):
    """1, 7, 8, 9, 13 and 16 blocks (the XCD remapping with per == 0, rem == 0 and both non-zero) whose last block holds
    1, 31, 33 or rows - 1 receivers."""
    shapes = apc.GRID_SHAPES_64 if apc.block_rows(k) == 64 else apc.GRID_SHAPES_32
    for nblocks, tail in shapes:
        src_cpu, blocks, n, table_rows = apc.grid_case_senders(k, nblocks, tail, seed=nblocks)
        kk, sl = (k if k in (8, 16) else 0), (width // 32 if width in (128, 256) else 0)
        assert _form(table_rows, n, k, width) == kk * 16 + sl
        src = src_cpu.to(DEV)
        plan = ops.AggregatePlan(src, n, k)
        apc.check_plan(plan.blob.cpu(), src_cpu, n, k)
        table_cpu = _table(table_rows, width, seed=nblocks)
        _, table = _device_table(table_cpu)
        got = _planned(table, src, plan, n, k, "rows")
        assert bool(torch.isfinite(got).all())
        _compare_three_ways(got, table_cpu, table, src_cpu, src, n, k, f"{nblocks} blocks, last of {tail}")


@pytest.mark.parametrize("case", [c for c in apc.FORM_CASES if c[3] % 16 != 0], ids=_ids)
def test_ghost_rows_in_every_32_bit_form(case):
    """table_rows = num_nodes + ghosts: the last table row, a ghost, carries values no other row has; every receiver that
    lists it must show them."""
    k, width, route, form = case
    src_cpu, blocks, n, table_rows = apc.form_case_senders(k, seed=k)
    assert route == "rows" and table_rows > n and _form(table_rows, n, k, width) == form
    listing = (src_cpu.view(n, k) == table_rows - 1).any(dim=1)
    assert int(listing.sum()) >= len(blocks) - 4                        # nearly every block reaches it
    table_cpu = _table(table_rows, width, seed=5) * 0.01
    table_cpu[table_rows - 1] = 1000.0 + torch.arange(width)
    src = src_cpu.to(DEV)
    plan = ops.AggregatePlan(src, n, k)
    _, table = _device_table(table_cpu)
    got = _planned(table, src, plan, n, k, route)
    assert bool((got[listing] > 900.0).all()) and bool((got[~listing].abs() < 100.0).all())
    _compare_three_ways(got, table_cpu, table, src_cpu, src, n, k, _ids(case))


@pytest.mark.parametrize("case", [c for c in apc.FORM_CASES if c[:3] in ((16, 128, "rows"), (8, 256, "rows"),
                                                                         (12, 128, "rows"), (16, 128, "norows"),
                                                                         (12, 96, "rows"))], ids=_ids)
def test_a_poisoned_row_reaches_exactly_the_receivers_that_list_it(case):
    """One table row set to NaN, +inf or -0.0: a row staged in LDS, a row of a direct-path block, a ghost row.  Exactly
    the receivers that list it change, and the others keep the clean run's bits (no stale or foreign LDS row)."""
    k, width, route, form = case
    src_cpu, blocks, n, table_rows = apc.form_case_senders(k, seed=k)
    assert _form(table_rows if route == "rows" else 0, n, k, width) == form
    rows = apc.block_rows(k)
    sets, counts = apc.plan_restated(src_cpu, n, k)
    staged = [b for b, c in enumerate(counts) if 33 <= c <= apc.STAGE_ROWS]
    direct = [b for b, c in enumerate(counts) if c < 0 or c > apc.STAGE_ROWS]
    assert staged and direct
    owned = lambda s: [int(i) for i in s if 0 < i < n]                   # not row 0 / the ghost that every block lists
    targets = {"staged": owned(sets[staged[0]])[-1], "direct": owned(sets[direct[-1]])[0], "ghost": table_rows - 1}
    src = src_cpu.to(DEV)
    plan = ops.AggregatePlan(src, n, k)
    table_cpu = _table(table_rows, width, seed=77)
    _, table = _device_table(table_cpu)
    clean = _planned(table, src, plan, n, k, route)
    for where, row in targets.items():
        listing = (src_cpu.view(n, k) == row).any(dim=1)
        assert 0 < int(listing.sum()) < n
        for value in (float("nan"), float("inf"), -0.0):
            poisoned_cpu = table_cpu.clone()
            poisoned_cpu[row] = value
            table[row] = value
            got = _planned(table, src, plan, n, k, route)
            what = f"{_ids(case)}: {where} row {row} = {value}"
            if value != value:
                assert torch.equal(torch.isnan(got).all(dim=1), listing) and not bool(torch.isnan(got[~listing]).any()), what
            elif value == float("inf"):
                assert torch.equal((got == float("inf")).all(dim=1), listing), what
                assert bool(torch.isfinite(got[~listing]).all()), what
            assert torch.equal(got[~listing].view(torch.int32), clean[~listing].view(torch.int32)), what
            _compare_three_ways(got, poisoned_cpu, table, src_cpu, src, n, k, what)
            table[row] = table_cpu[row].to(DEV)
    assert torch.equal(_planned(table, src, plan, n, k, route).view(torch.int32), clean.view(torch.int32))


@pytest.mark.parametrize("k", [16, 5])
def test_hash_table_of_the_plan_build_under_collisions(k):
    """Blocks whose senders all share one hash value (a probe chain of 56), and whose senders hash to 4094, 4095 and 0 (the
    chain wraps past the last slot into occupied ones), between ordinary blocks: the plan is checked field by field and
    the sums three ways (a width-32 table of 2^18 rows)."""
    src_cpu, blocks, n, table_rows = apc.hash_case_senders(k)
    width = 32
    assert _form(table_rows, n, k, width) == (k if k in (8, 16) else 0) * 16
    src = src_cpu.to(DEV)
    plan = ops.AggregatePlan(src, n, k)
    apc.check_plan(plan.blob.cpu(), src_cpu, n, k)
    table_cpu = _table(table_rows, width, seed=k)
    table = table_cpu.to(DEV)
    got = _planned(table, src, plan, n, k, "rows")
    _compare_three_ways(got, table_cpu, table, src_cpu, src, n, k, f"hash blocks, k = {k}")


def test_one_plan_serves_tables_of_different_widths_and_values():
    k = 16
    src_cpu, blocks, n, table_rows = apc.form_case_senders(k, seed=k)
    src = src_cpu.to(DEV)
    plan = ops.AggregatePlan(src, n, k)
    before = plan.blob.clone()
    for width, seed in ((128, 1), (64, 2), (256, 3), (128, 4)):
        table_cpu = _table(table_rows, width, seed)
        table = table_cpu.to(DEV)
        got = ops.aggregate(table, src, None, n, k, plan=plan).cpu()          # the route the model takes
        again = ops.aggregate(table, src, None, n, k, plan=plan).cpu()
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        assert torch.equal(got.view(torch.int32), _planned(table, src, plan, n, k, "rows").view(torch.int32))
        _compare_three_ways(got, table_cpu, table, src_cpu, src, n, k, f"reuse, width {width}")
    assert torch.equal(plan.blob, before)                                     # the kernel only reads its plan


def test_no_receivers_is_ok_and_writes_nothing():
    k, width = 16, 128
    src_cpu, blocks, n, table_rows = apc.form_case_senders(k, seed=k)
    src = src_cpu.to(DEV)
    plan = ops.AggregatePlan(src, n, k)
    table = _table(table_rows, width, 1).to(DEV)
    buf, out = _guarded(n, width)
    bits = buf.view(torch.int32)                                              # all of it the sentinel, `out` included
    lib = _lib.load()
    rc = lib.cgnn_aggregate_planned_rows(table.data_ptr(), table_rows, src.data_ptr(), plan.blob.data_ptr(), 0, k, width,
                                         out.data_ptr(), _lib.stream_ptr(table.device))
    assert rc == 0
    rc = lib.cgnn_aggregate_planned(table.data_ptr(), src.data_ptr(), plan.blob.data_ptr(), 0, k, width, out.data_ptr(),
                                    _lib.stream_ptr(table.device))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((bits == SENTINEL).all())


def test_the_4_gib_edge_of_the_32_bit_forms():
    """Width 128: 8,388,605 table rows is the largest table of the 32-bit form (the last row's pieces lie within 1.5 KiB of
    2^32, where an offset plus a slice offset could wrap), 8,388,606 the smallest of the 64-bit form.  8,192 receivers,
    k = 16, senders at row 0, at the last row and all over the table, blocks with more and fewer than 352 distinct
    senders.  The referenced rows are gathered on the device and summed on the CPU in the kernel's order."""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 1024 ** 3:
        pytest.skip(f"needs 12 GB of free device memory for a 4.3-GB table, its plain gather and slack; {free >> 30} GB free")
    k, width, n = apc.EDGE_4G["k"], apc.EDGE_4G["width"], apc.EDGE_4G["num_nodes"]
    big = torch.empty(apc.EDGE_4G["rows_64bit"], width, device=DEV)
    step = 1 << 20
    gen = torch.Generator(device=DEV).manual_seed(4)
    for r0 in range(0, big.shape[0], step):
        big[r0: r0 + step].normal_(generator=gen)
    for table_rows, form in ((apc.EDGE_4G["rows_32bit"], 16 * 16 + 4), (apc.EDGE_4G["rows_64bit"], 16 * 16)):
        assert _form(table_rows, n, k, width) == form
        table = big[:table_rows]
        src_cpu, blocks = apc.edge_4g_senders(table_rows)
        assert int(src_cpu.max()) == table_rows - 1 and int(src_cpu.min()) == 0
        src = src_cpu.to(DEV)
        plan = ops.AggregatePlan(src, n, k)
        apc.check_plan(plan.blob.cpu(), src_cpu, n, k)
        got = _planned(table, src, plan, n, k, "rows")
        rows = table[src.long()].cpu().view(n, k, width)                      # 64 MB: the referenced rows only
        want = apc.sum_rows_kernel_order(rows)
        assert apc.same_bits(got, want), f"{table_rows} rows: receivers {_differing_rows(got, want)} differ"
        plain = ops.aggregate(table, src, None, n, k).cpu()
        assert apc.same_bits(got, plain), f"{table_rows} rows: receivers {_differing_rows(got, plain)} differ from cgnn_aggregate"
        err = (got.double() - rows.double().sum(dim=1)).abs()
        assert bool((err <= (k - 1) * 2.0 ** -24 * rows.double().abs().sum(dim=1)).all())
        assert bool(torch.isfinite(got).all())
        del plan, src, rows
