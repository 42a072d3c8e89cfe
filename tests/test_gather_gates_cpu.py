"""CPU, every run: the launch geometry of the gather / scatter / CSR / relayout kernels restated in tests/gather_checks.py --
the finders pinned at 256 compute units, xcd_work_range covering [0, total) once on every grid, the library's CSR workspace
size -- the builders' own properties (the order probe distinguishes orders, the exact-range assertion fires, TILED32 is a
bijection), and the exact gate tested on itself: stand-ins that follow the restated geometry pass ``assert_exact`` at the
shapes tests/test_gpu_gather_gates.py uses, and every planted defect -- an eighth's end rounded down, an end flush that drops
the wave's last group, a scan without block offsets, an insertion sort cut off at 47, pad rows left alone, a scatter that
writes one row too many, a remainder loop that skips the last edge -- is rejected there."""
import pytest
import torch

import gather_checks as gc
import reduction_checks as rc
from cosmology_gnn_simulation_amd import _lib

CUS = 256


def _passes(got, want, what, block=None):
    try:
        rc.assert_exact(got, want, what, block)
    except AssertionError:
        return False
    return True


# ---- pinned numbers ------------------------------------------------------------------------------------------------------------
def test_finders_at_256_compute_units():
    first = lambda kind: [gc.first_second_pass(kind, w, CUS) for w in (4, 32, 36, 256)]
    assert first("fixedk_rows") == first("fixedk_tiled") == [4194305, 524289, 466034, 65537]
    assert first("relayout") == [2097153, 262145, 232993, 32769]
    assert first("gather_rows") == first("scatter_rows") == [2097153, 262145, 233017, 32769]
    assert gc.first_second_pass("gather_rows", 3, CUS) == 699051 and gc.first_second_pass("scatter_rows", 260, CUS) == 32264
    assert gc.first_total_beyond_8_blocks(CUS) == 2049
    at = lambda w: [gc.edge_counts(w)[k] for k in ("group+0", "wave+0", "block+0")]
    assert [at(w) for w in gc.GENERAL_WIDTHS] == [[1312, 1280, 2048], [672, 640, 1024], [352, 320, 512], [192, 160, 256],
                                                  [5136, 5120, 8192], [5136, 5120, 8192]]
    assert set(gc.edge_counts(32)) == {f"{b}{d:+d}" for b in ("group", "wave", "block") for d in (-1, 0, 1)}
    assert [gc.fixedk_sizes(w, CUS)["ragged_eighths"] for w in gc.FIXEDK_WIDTHS] == [6145, 769, 683, 193, 97]
    assert [gc.scan_blocks(m) for m in gc.CSR_M] == [1, 1, 1, 1, 2, 2, 3, 4]


def test_finders_return_the_first_size_of_their_branch():
    for cus in (64, 256, 304):
        for kind, (cap, xcd, per_row) in gc.KINDS.items():
            for w in (4, 36, 256) + ((3,) if kind.endswith("_rows") and kind != "fixedk_rows" else ()):
                n = gc.first_second_pass(kind, w, cus)
                rows = (lambda v: gc.tiled_rows(v)) if kind == "relayout" else (lambda v: v)
                assert gc.passes(*gc.grid_for(kind, rows(n), w, cus), xcd) == 2
                assert gc.passes(*gc.grid_for(kind, rows(n - 1), w, cus), xcd) == 1
    for w in gc.GENERAL_WIDTHS:
        counts, geo = gc.edge_counts(w), gc.general_geometry
        for name, per in (("group", "groups"), ("wave", None), ("block", "blocks")):
            e = counts[f"{name}+0"]
            assert e % geo(w, e)[f"{name}_edges"] == 0 and counts[f"{name}-1"] == e - 1 and counts[f"{name}+1"] == e + 1
            if per:
                assert geo(w, e - 1)[per] == geo(w, e)[per] == geo(w, e + 1)[per] - 1
        if w in gc.SCATTER_WIDTHS:
            e = counts["wave+0"]
            assert geo(w, e)["waves"] == geo(w, e + 1)["waves"] - 1 and geo(w, e)["blocks"] == 2 and geo(w, counts["block+0"])["blocks"] == 2
            assert geo(w, 1)["lpr"] * geo(w, 1)["gpw"] == 64 and geo(w, 1)["steps"] * gc.SCATTER_U == gc.SCATTER_EPG


def test_the_fixed_k_launcher_never_takes_the_plain_stride():
    """blocks_for_xcd returns a multiple of 8 whatever the total: through cgnn_aggregate the eighths branch is the only one."""
    for cus in (1, 7, 8, 64, 256, 304):
        for total in list(range(0, 5000, 7)) + [1 << 20, (1 << 22) + 5, 1 << 30]:
            nb = gc.blocks_for_xcd(total, gc.CAP_FIXEDK, cus)
            assert nb % 8 == 0 and nb >= 8
    assert gc.blocks_for(0, 32, CUS) == 1 and gc.blocks_for(257, 32, CUS) == 2 and gc.blocks_for(1 << 30, 32, CUS) == 32 * CUS


def test_restated_csr_workspace_matches_the_library():
    lib = _lib.load()
    for rows in [m - 1 for m in gc.CSR_M] + [63, 64, 500, 100000, 1 << 22]:
        assert gc.csr_workspace_bytes(rows) == lib.cgnn_csr_workspace_bytes(rows), rows


# ---- geometry ------------------------------------------------------------------------------------------------------------------
TOTALS = (0, 1, 5, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 2055, 6145, 6147)


def test_xcd_work_range_visits_every_item_once():
    for nb in list(range(1, 25)):
        for total in TOTALS:
            seen = [0] * total
            for b in range(nb):
                for tid in range(gc.BLOCK):
                    for gid in gc.xcd_work_range(total, nb, b, tid):
                        seen[gid] += 1                           # an index outside [0, total) raises (or, negative, counts twice)
            assert seen == [1] * total, (nb, total)
            assert gc.xcd_visits(total, nb).tolist() == seen, (nb, total)
            if nb % 8 == 0:                                      # the eighths are [0, total) cut in order
                assert rc.covers_once([(total * x // 8, total * (x + 1) // 8) for x in range(8)], total)
                if total % 8:
                    assert not bool((gc.xcd_visits(total, nb, "end_rounded_down") == 1).all())
    for total in (1, 2049, 2048 * 256 - 1, 2048 * 256 + 5, 3 * 2048 * 256 + 9):   # 2048 workgroups: one, and more than one, trip
        assert bool((gc.xcd_visits(total, 2048) == 1).all()), total
    for total in (2048 * 256 * 8, 65537 * 64, 466034 * 9, 65537 * 64 + 3):           # the capped grid of 256 compute units
        assert gc.blocks_for_xcd(total, gc.CAP_FIXEDK, CUS) == 8 * 2048
        assert bool((gc.xcd_visits(total, 8 * 2048) == 1).all()), total
    for nb in (1, 3, 8, 24):                                                      # the plain loop of the other kernels
        for total in TOTALS:
            seen = sorted(g for b in range(nb) for tid in range(gc.BLOCK) for g in gc.plain_work_range(total, nb, b, tid))
            assert seen == list(range(total))


# ---- builders ------------------------------------------------------------------------------------------------------------------
def test_order_probes_tell_the_orders_apart():
    for m in (4, 5, 8, 9, 16, 17):
        a = gc.probe_addends(m)
        assert a[0, :4].tolist() == list(gc.PROBE) and bool((a.double().sum(1) == 2).all())     # exactly 2: no order gives it but reverse
        doc = gc.documented_sum(a)
        others = [gc.reverse_sum(a)] + ([gc.sequential_sum(a)] if m in (8, 16) else [gc.pairwise_sum(a)])
        for other in others:
            assert not torch.equal(doc, other), m
        assert float(doc[0]) == (1.0 if m in (8, 16) else 0.0)
        assert torch.equal(gc.PROBE_TABLE[gc.probe_gather(a).long()].view(a.shape), a)
    a = gc.probe_addends(4)
    assert (float(gc.sequential_sum(a)[0]), float(gc.reverse_sum(a)[0]), float(gc.pairwise_sum(a)[0])) == (0.0, 2.0, 1.0)
    # the own row first (halo_return_add): 2^24 as `first`, then 1, 1, -2^24; taken last it gives 2
    first, rest = a[:1, 0], a[:1, 1:]
    assert float(gc.sequential_sum(rest, first)[0]) == 0.0 and float(gc.sequential_sum(rest)[0] + first[0]) == 2.0
    # (add1 + add2) + sum against add1 + (add2 + sum) and (sum + add1) + add2
    one, big = torch.tensor(1.0), torch.tensor(gc.BIG)
    assert float((one + one) + big) == gc.BIG + 2 and float(one + (one + big)) == gc.BIG and float((big + one) + one) == gc.BIG


def test_the_exact_range_assertion_fires():
    gc.check_contributions((1 << 22) - 1)
    with pytest.raises(AssertionError, match="no float32 integer"):
        gc.check_contributions(1 << 22)
    with pytest.raises(AssertionError):
        gc.aggregate_reference(torch.full((4, 4), 0.5), None, torch.zeros(4, dtype=torch.int64), 1)
    with pytest.raises(AssertionError, match="no float32 values"):
        gc.to_f32_exact(torch.tensor([(1 << 24) + 1]))
    p = gc.aggregate_problem(1, 7, 4, gc.fixedk_dst(7, 3), senders="random", table_rows=9)
    assert torch.isnan(p["table"].full[:rc.PAD_ROWS]).all() and torch.isnan(p["table"].full[-rc.PAD_ROWS:]).all()
    assert p["table"].full.shape[0] == 9 + 2 * rc.PAD_ROWS and float(p["values"].abs().max()) <= 4
    assert float(p["out"].full.min()) >= gc.PATTERN_BASE > float(p["want"].abs().max())


def test_tiled32_is_a_bijection_beside_the_pad_rows():
    for n, width in ((1, 32), (31, 64), (32, 32), (33, 256), (4097, 64)):
        off = gc.tiled_offsets(n, width).reshape(-1)
        pads = gc.tiled_offsets(gc.tiled_rows(n), width, first_row=n).reshape(-1)
        both = torch.cat([off, pads]).sort().values
        assert torch.equal(both, torch.arange(gc.tiled_rows(n) * width))
        assert off.numel() == n * width and pads.numel() == (gc.tiled_rows(n) - n) * width
        x = torch.arange(n * width, dtype=torch.float32).view(n, width)
        buf = gc.to_tiled(x, rc.NAN)
        assert int(torch.isnan(buf).sum()) == pads.numel() and torch.equal(buf[off].view(n, width), x)
    # the address map as include/cgnn.h words it
    row, f, width = 70, 32 * 3 + 8 * 2 + 4 * 1 + 3, 256
    assert int(gc.tiled_offsets(row + 1, width)[row, f]) == 2 * 32 * width + ((4 * 3 + 2) * 64 + 32 * 1 + 6) * 4 + 3


def test_edge_lists_hold_what_they_are_named_for():
    for w in gc.GENERAL_WIDTHS:
        geo = gc.general_geometry(w, 1)
        for e in gc.edge_counts(w).values():
            for u in range(4):
                dst, n = gc.edge_list(f"change_at_{u}", e, w)
                changes = (torch.nonzero(dst[1:] != dst[:-1])[:, 0] + 1) % 4
                assert set(changes.tolist()) == {u} and int(dst.max()) < n
            dst, n = gc.edge_list("every_edge", e, w)
            assert bool((dst[1:] != dst[:-1]).all())
            dst, n = gc.edge_list("one_destination", e, w)
            assert len(set(dst.tolist())) == 1
            dst, n = gc.edge_list("straddle", e, w)
            for name in ("group_edges", "wave_edges", "block_edges"):
                assert geo[name] in gc.runs_across(dst, geo[name]) or geo[name] + 3 > e
            assert all(geo[name] + 3 <= e for name in ("group_edges", "wave_edges", "block_edges"))
            dst, n = gc.edge_list("returns", e, w)
            assert dst[:12].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 0, 0, 0]
            dst, n = gc.edge_list("ends", e, w)
            assert set(dst.tolist()) == {0, n - 1}


def test_csr_key_lists_hold_what_they_are_named_for():
    for rows, last in gc.csr_rows_cases():
        k = gc.csr_keys(rows, rows, last)
        counts = torch.bincount(k["key"].long(), minlength=max(rows, 1))[:rows]
        if rows >= 58:
            planted = {(length, form) for length, form in k["planted"].values()}
            assert planted == {(length, form) for length in gc.PLANTED_LENGTHS for form in gc.VALUE_FORMS}
            assert all(int(counts[r]) == length for r, (length, _) in k["planted"].items())
            assert int(counts[0]) == 0 and (int(counts[-1]) == 0) == (last == "empty")
        if rows >= 2 * gc.SCAN_ITEMS and (last == "empty" or rows > 2 * gc.SCAN_ITEMS):
            assert int(counts[gc.SCAN_ITEMS:2 * gc.SCAN_ITEMS].sum()) == 0          # a whole scan block of zero counts
        row_ptr, col = gc.csr_reference(k["key"], k["val"], rows)
        assert int(row_ptr[-1]) == k["key"].numel() and row_ptr.numel() == rows + 1
        assert k["key"].numel() == 0 or 0 <= int(k["val"].min()) <= int(k["val"].max()) < k["table_rows"]
        for r, (length, form) in list(k["planted"].items())[::5]:
            seg = col[int(row_ptr[r]):int(row_ptr[r + 1])]
            assert torch.equal(seg, k["val"][k["key"] == r].sort().values)
            if form == "duplicates" and length >= 7:
                assert len(set(seg.tolist())) < length
    assert any(rows == 2 * gc.SCAN_ITEMS for rows, _ in gc.csr_rows_cases()) and any(rows > 2 * gc.SCAN_ITEMS for rows, _ in gc.csr_rows_cases())


# ---- the gates on themselves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", gc.FIXEDK_WIDTHS)
def test_gate_on_the_fixed_k_stand_in(width):
    caught = {}
    for name, n in gc.fixedk_sizes(width, CUS).items():
        for k in gc.FIXEDK_KS:
            p = gc.aggregate_problem(k + n, n, width, gc.fixedk_dst(n, k), senders="random" if k != 17 else None)
            want = p["out"].expected(p["want"])
            assert _passes(gc.standin_fixedk(p, k, CUS), want, (name, k), p["out"].block)
            caught[name, k] = not _passes(gc.standin_fixedk(p, k, CUS, defect="end_rounded_down"), want, (name, k), p["out"].block)
    odd_chunks = (width // 4) % 8 != 0
    assert all(hit == odd_chunks for hit in caught.values()), caught       # total % 8 != 0 exists at widths 4 and 36 only
    # a row read from before the table is NaN and fails
    p = gc.aggregate_problem(1, 5, width, gc.fixedk_dst(5, 3), senders="random")
    p["values"] = p["table"].full[rc.PAD_ROWS - 1:]
    assert not _passes(gc.standin_fixedk(p, 3, CUS), p["out"].expected(p["want"]), "shifted", p["out"].block)


def test_gate_on_the_fixed_k_stand_in_at_the_second_pass():
    """The sizes of the two second-pass cases of the GPU file at 256 compute units, at width 36 (the same work items per
    eighth as width 256 to within one, a ninth of the bytes): a second trip exists, and the defect is caught there."""
    n = gc.first_second_pass("fixedk_rows", 36, CUS)
    total, nb = gc.grid_for("fixedk_rows", n, 36, CUS)
    assert nb == 8 * 2048 and gc.passes(total, nb, True) == 2 and total % 8
    p = gc.aggregate_problem(3, n, 36, gc.fixedk_dst(n, 3), senders="random")
    want = p["out"].expected(p["want"])
    assert _passes(gc.standin_fixedk(p, 3, CUS), want, "second pass", p["out"].block)
    assert not _passes(gc.standin_fixedk(p, 3, CUS, defect="end_rounded_down"), want, "second pass", p["out"].block)
    assert gc.passes(*gc.grid_for("fixedk_rows", gc.first_second_pass("fixedk_rows", 256, CUS), 256, CUS), True) == 2


@pytest.mark.parametrize("width", gc.GENERAL_WIDTHS)
def test_gate_on_the_general_stand_in(width):
    form = {32: "gather", 64: "edge", 128: "tiled", 256: "gather", 4: "edge", 36: "gather"}[width]
    for cname, e in gc.edge_counts(width).items():
        for lname in gc.EDGE_LISTS:
            dst, n = gc.edge_list(lname, e, width)
            p = gc.aggregate_problem(e, n, width, dst, senders="random" if form == "gather" else None, table_rows=n + 3)
            want = p["out"].expected(p["want"])
            assert _passes(gc.standin_general(p), want, (cname, lname), p["out"].block)
            if width in gc.SCATTER_WIDTHS:
                got = gc.standin_general(p, defect="flush_drops_last_group")
                assert not _passes(got, want, (cname, lname), p["out"].block), (cname, lname)
    dst, n = gc.edge_list("one_destination", 1 << 12, width)               # 2^12 edges into one row
    p = gc.aggregate_problem(5, n, width, dst, senders="random", table_rows=64)
    assert _passes(gc.standin_general(p), p["out"].expected(p["want"]), "2^12", p["out"].block)
    for e in (0, 1):
        p = gc.aggregate_problem(e, 3, width, torch.zeros(e, dtype=torch.int64))
        assert _passes(gc.standin_general(p), p["out"].expected(p["want"]), e, p["out"].block)


@pytest.mark.parametrize("rows,last", gc.csr_rows_cases())
def test_gate_on_the_csr_stand_in(rows, last):
    k = gc.csr_keys(rows, rows, last)
    for val in (k["val"], None):
        want_ptr, want_col = gc.csr_reference(k["key"], val, rows)
        got_ptr, got_col = gc.standin_csr_build(k["key"], val, rows)
        assert torch.equal(got_ptr, want_ptr) and torch.equal(got_col, want_col)
        bad_ptr, bad_col = gc.standin_csr_build(k["key"], val, rows, defect="scan_without_offsets")
        assert (not torch.equal(bad_ptr, want_ptr)) == (rows + 1 > gc.SCAN_ITEMS)
        bad_ptr, bad_col = gc.standin_csr_build(k["key"], val, rows, defect="insertion_cut_at_47")
        assert (not torch.equal(bad_col, want_col)) == (rows >= 58)


@pytest.mark.parametrize("width", (4, 36, 128))
def test_gate_on_the_segment_sum_stand_ins(width):
    rows = 2048
    k = gc.csr_keys(7, rows, "full")
    row_ptr, col = gc.csr_reference(k["key"], k["val"], rows)
    gen = torch.Generator().manual_seed(width)
    table = gc.Padded(rc.int_matrix(gen, k["table_rows"], width, "cpu"))
    add1, add2 = rc.int_matrix(gen, rows, width, "cpu"), rc.int_matrix(gen, rows, width, "cpu")
    for a, b in ((0, rows), (3, 90), (5, 5), (rows - 1, rows)):
        want = gc.segment_sum_reference(table.values, row_ptr, col, a, b)
        for a1, a2 in ((None, None), (add1[:b - a], None), (None, add2[:b - a]), (add1[:b - a], add2[:b - a])):
            full = want + (0 if a1 is None else a1) + (0 if a2 is None else a2)
            got = gc.standin_segment_sum(table.values, row_ptr, col, a, b, add1=a1, add2=a2)
            assert _passes(got, full, (a, b))
            bad = gc.standin_segment_sum(table.values, row_ptr, col, a, b, add1=a1, add2=a2, defect="remainder_skips_last_edge")
            lengths = (row_ptr[1:] - row_ptr[:-1])[a:b]
            assert (not _passes(bad, full, (a, b))) == bool((lengths % 4 != 0).any())
    # halo_return_add: segment lengths 0 ... 9, the own row first
    hrows, seg_ptr, hcol = gc.halo_plan(width, 64, 40)
    ret = rc.int_matrix(gen, 40, width, "cpu")
    own = table.values[:64]
    want = own[hrows.long()] + gc.segment_sum_reference(ret, seg_ptr, hcol, 0, hrows.numel())
    assert _passes(gc.standin_segment_sum(ret, seg_ptr, hcol, 0, hrows.numel(), first=own[hrows.long()]), want, "halo")
    assert not _passes(gc.standin_segment_sum(ret, seg_ptr, hcol, 0, hrows.numel(), first=own[hrows.long()],
                                              defect="remainder_skips_last_edge"), want, "halo")
    assert sorted(set((seg_ptr[1:] - seg_ptr[:-1]).tolist())) == list(range(10))


def test_order_probe_through_the_segment_sum_stand_in():
    """The CSR form of the probe: row i sums table rows 4 i ... 4 i + 3 in ascending p."""
    a = gc.probe_addends(4)
    table = a.reshape(-1, 1) * gc.column_factors(8)[None, :]
    row_ptr = torch.arange(0, 4 * a.shape[0] + 1, 4, dtype=torch.int32)
    col = torch.arange(4 * a.shape[0], dtype=torch.int32)
    got = gc.standin_segment_sum(table, row_ptr, col, 0, a.shape[0])
    assert torch.equal(got, gc.sequential_sum(a)[:, None] * gc.column_factors(8)[None, :])
    assert not torch.equal(got, gc.reverse_sum(a)[:, None] * gc.column_factors(8)[None, :])


@pytest.mark.parametrize("width", gc.RELAYOUT_WIDTHS)
def test_gate_on_the_relayout_stand_in(width):
    for n in gc.RELAYOUT_N + (gc.first_second_pass("relayout", 256, CUS),):
        if n > 4097 and width != 256:
            continue
        x = rc.int_matrix(torch.Generator().manual_seed(n), n, width, "cpu")
        tiled_nan, tiled_zero = gc.to_tiled(x, rc.NAN), gc.to_tiled(x, 0.0)
        for src, ft, tt, want in ((x.reshape(-1), False, True, tiled_zero), (tiled_nan, True, False, x.reshape(-1)),
                                  (tiled_nan, True, True, tiled_zero), (x.reshape(-1), False, False, x.reshape(-1))):
            dst = torch.full((gc.tiled_rows(n) * width + 64,), rc.NAN)
            want_full = dst.clone()
            want_full[:want.numel()] = want
            assert _passes(gc.standin_relayout(src, ft, dst.clone(), tt, n, width), want_full, (n, ft, tt), slice(0, 0))
            bad = gc.standin_relayout(src, ft, dst.clone(), tt, n, width, defect="pads_left_alone")
            assert (not _passes(bad, want_full, (n, ft, tt), slice(0, 0))) == (tt and n % 32 != 0)


@pytest.mark.parametrize("width", gc.ROWS_WIDTHS)
def test_gate_on_the_row_stand_ins(width):
    for n_idx in gc.ROWS_N_IDX:
        p = gc.rows_problem(n_idx + width, n_idx, width)
        got = gc.standin_gather_rows(p["table"].values, p["idx_full"], n_idx, p["out"].full.clone()[rc.PAD_ROWS:])
        assert _passes(got, p["out"].expected(p["gathered"])[rc.PAD_ROWS:], n_idx, slice(0, n_idx))
        want = p["dest"].full.clone()
        want[rc.PAD_ROWS:][p["perm"].long()] = p["rows"].values
        got = p["dest"].full.clone()
        gc.standin_scatter_rows(p["rows"].full[rc.PAD_ROWS:], p["perm_full"], n_idx, got[rc.PAD_ROWS:])
        assert _passes(got, want, n_idx, p["dest"].block)
        bad = p["dest"].full.clone()
        gc.standin_scatter_rows(p["rows"].full[rc.PAD_ROWS:], p["perm_full"], n_idx, bad[rc.PAD_ROWS:], defect="one_row_too_many")
        assert not _passes(bad, want, n_idx, p["dest"].block)
