"""CPU: the restatements of tests/aggregate_plan_checks.py checked against themselves -- sender lists with chosen block
contents, the reader of the plan blob, the kernel-order sum against float64 -- and ``cgnn_aggregate_planned_form``, the
one place that chooses among the nine forms of ``aggregate_planned_kernel``, on each side of its limits (host only)."""
import os

import numpy as np
import pytest
import torch

import aggregate_plan_checks as apc
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib

ENTRIES = ("cgnn_aggregate_planned_form",)


def _distinct_per_block(src, n, k):
    return [len(s) for s in apc.plan_restated(src, n, k)[0]]


def _assert_sender_list(src, blocks, n, k, table_rows):
    assert src.dtype == torch.int32 and src.shape == (n * k,)
    assert int(src.min()) >= 0 and int(src.max()) < table_rows
    assert _distinct_per_block(src, n, k) == list(blocks)


@pytest.mark.parametrize("k", sorted({c[0] for c in apc.FORM_CASES}))
def test_make_senders_delivers_the_block_contents_of_the_form_cases(k):
    src, blocks, n, table_rows = apc.form_case_senders(k, seed=k)
    _assert_sender_list(src, blocks, n, k, table_rows)
    rows = apc.block_rows(k)
    assert set(apc.block_spec(k)) <= set(blocks) and rows * k in blocks       # all distinct is among them
    assert n % rows == rows - 1                                               # a partial last block
    g = src.view(n, k)
    for b in apc._ends(blocks):                                               # row 0 and the last (ghost) row
        mine = g[b * rows: (b + 1) * rows]
        assert bool((mine == 0).any()) and bool((mine == table_rows - 1).any())
    assert int((g == g[:, :1]).all(dim=1).sum()) >= 1                         # a receiver with k equal senders
    assert int((g == torch.arange(n).view(n, 1)).any(dim=1).sum()) >= 1       # a receiver that lists itself
    expect = {1: [1, 2, 31, 32], 5: [1, 2, 31, 32, 33, 160], 11: [1, 2, 31, 32, 33, 351, 352],
              12: [1, 2, 31, 32, 33, 351, 352, 353, 384], 8: [1, 2, 31, 32, 33, 351, 352, 353, 511, 512],
              16: [1, 2, 31, 32, 33, 351, 352, 353, 511, 512, 513, 1024],
              32: [1, 2, 31, 32, 33, 351, 352, 353, 511, 512, 513, 1024]}
    assert apc.block_spec(k) == expect[k]


def test_every_form_has_a_case_and_the_cases_include_the_odd_widths():
    assert {c[3] for c in apc.FORM_CASES} == apc.ALL_FORMS and len(apc.ALL_FORMS) == 9
    assert {96, 160} <= {c[1] for c in apc.FORM_CASES} and 1 in {c[0] for c in apc.FORM_CASES}


@pytest.mark.parametrize("k,width", apc.GRID_FORMS)
def test_make_senders_delivers_the_block_contents_of_the_grid_cases(k, width):
    shapes = apc.GRID_SHAPES_64 if apc.block_rows(k) == 64 else apc.GRID_SHAPES_32
    assert [s[0] for s in shapes] == [1, 7, 8, 9, 13, 16]
    tails = {s[1] for s in shapes}
    assert tails == ({1, 31, 33, 63} if apc.block_rows(k) == 64 else {1, 31})
    for nblocks, tail in shapes:
        src, blocks, n, table_rows = apc.grid_case_senders(k, nblocks, tail, seed=nblocks)
        assert len(blocks) == nblocks and n % apc.block_rows(k) == tail
        _assert_sender_list(src, blocks, n, k, table_rows)


@pytest.mark.parametrize("k", [16, 5])
def test_make_senders_delivers_the_hash_blocks(k):
    src, blocks, n, table_rows = apc.hash_case_senders(k)
    _assert_sender_list(src, blocks, n, k, table_rows)
    rows = apc.block_rows(k)
    sets, _ = apc.plan_restated(src, n, k)
    assert len(sets[1]) >= 48 and set(apc.hash_of(sets[1]).tolist()) == {apc.HASH_ONE}
    hashes = apc.hash_of(sets[3])
    assert set(hashes.tolist()) == {4094, 4095, 0} and int((hashes >= 4094).sum()) == 80
    assert n == 6 * rows + 20


def test_ids_with_hash_restates_the_kernels_hash():
    ids = apc.ids_with_hash(4095, 48, 1 << 18)
    assert len(ids) == 48 and len(set(ids.tolist())) == 48 and ids.max() < 1 << 18
    for i in ids[:5].tolist() + [1, 40503, (1 << 31) - 1]:
        assert int(apc.hash_of([i])[0]) == ((i * 2654435761) % (1 << 32)) >> 20
    assert all(int(h) == 4095 for h in apc.hash_of(ids))
    with pytest.raises(ValueError):
        apc.ids_with_hash(7, 48, 1000)
    with pytest.raises(ValueError):
        apc.ids_with_hash(4096, 1, 1000)


def test_make_senders_at_the_4_gib_edge():
    for table_rows in (apc.EDGE_4G["rows_32bit"], apc.EDGE_4G["rows_64bit"]):
        src, blocks = apc.edge_4g_senders(table_rows)
        _assert_sender_list(src, blocks, 8192, 16, table_rows)
        assert int(src.min()) == 0 and int(src.max()) == table_rows - 1
        assert min(blocks) < 352 < max(blocks)
        quarters = np.bincount((src.numpy().astype(np.int64) * 4 // table_rows), minlength=4)
        assert quarters.min() > 8192 * 16 // 32                               # rows from all over the table


def test_make_senders_refuses_what_cannot_be_met():
    with pytest.raises(ValueError):
        apc.make_senders([161], 5, 1000, 32, 0)                               # U > rows * k
    with pytest.raises(ValueError):
        apc.make_senders([10, 6], 5, 1000, 33, 0)                             # ... of the partial block
    with pytest.raises(ValueError):
        apc.make_senders([0], 5, 1000, 32, 0)
    with pytest.raises(ValueError):
        apc.make_senders([10], 5, 1000, 64, 0)                                # two blocks, one count
    with pytest.raises(ValueError):
        apc.make_senders([40], 5, 1000, 32, 0, whole_table=False)             # 40 distinct ids below 32
    with pytest.raises(ValueError):
        apc.make_senders([1], 5, 1000, 32, 0, whole_table=True, ends=(0,))    # both ends in one id
    with pytest.raises(ValueError):
        apc.make_senders([160], 5, 1000, 32, 0, whole_table=True, same_row=(3,))  # all distinct and five equal
    with pytest.raises(ValueError):
        apc.make_senders([3], 5, 1000, 32, 0, ids={0: [1, 1, 2]})
    src = apc.make_senders([156], 5, 1000, 32, 0, whole_table=True, same_row=(3,))
    assert _distinct_per_block(src, 32, 5) == [156] and len(set(src.view(32, 5)[3].tolist())) == 1
    assert not torch.equal(apc.make_senders([20], 5, 1000, 32, 1), apc.make_senders([20], 5, 1000, 32, 2))
    assert torch.equal(apc.make_senders([20], 5, 1000, 32, 1), apc.make_senders([20], 5, 1000, 32, 1))
    assert int(apc.make_senders([20], 5, 1000, 32, 1).max()) < 32             # the receivers' rows only, by default


@pytest.mark.parametrize("k", [16, 5])
def test_check_plan_accepts_the_restated_blob_and_rejects_each_defect(k):
    rows = apc.block_rows(k)
    blocks = [u for u in (40, 1, min(513, rows * k), 33, 7) if u <= rows * k]
    n = (len(blocks) - 1) * rows + 9
    src = apc.make_senders(blocks, k, n + 600, n, 3, whole_table=True)
    good = apc.blob_from_restatement(src, n, k, seed=1)
    assert good.size == _lib.load().cgnn_aggregate_plan_bytes(n, k)           # the blob's layout is the library's
    apc.check_plan(good, src, n, k)
    apc.check_plan(torch.from_numpy(good.copy()), src, n, k)
    _, counts = apc.plan_restated(src, n, k)
    assert counts.tolist() == [u if u <= 512 else -1 for u in blocks]

    def broken(change):
        raw = good.copy()
        change(*apc.split_blob(raw, n, k))
        with pytest.raises(AssertionError):
            apc.check_plan(raw, src, n, k)

    def wrong_local(count, unique, local):
        e = 3 * rows * k + 4                                                  # an edge of block 3 (33 senders)
        local[e] = (local[e] + 1) % 33

    def local_past_count(count, unique, local):
        local[5] = 40

    def duplicated_unique(count, unique, local):
        unique[0, 7] = unique[0, 8]

    def foreign_unique(count, unique, local):
        unique[0, 7] = n + 599 if n + 599 not in unique[0, :40] else n + 598

    def wrong_count(count, unique, local):
        count[3] = 34

    def count_not_minus_one(count, unique, local):
        count[1] = -1

    for change in (wrong_local, local_past_count, duplicated_unique, foreign_unique, wrong_count, count_not_minus_one):
        broken(change)
    # nothing is required of unique / local where count is -1
    if -1 in counts.tolist():
        raw = good.copy()
        count, unique, local = apc.split_blob(raw, n, k)
        b = counts.tolist().index(-1)
        unique[b] = 12345
        local[b * rows * k: (b + 1) * rows * k] = 60000
        apc.check_plan(raw, src, n, k)


@pytest.mark.parametrize("k", [1, 5, 8, 11, 12, 16, 32])
def test_kernel_order_sum_is_within_k_minus_one_roundings_of_float64(k):
    """|sum_kernel_order - sum_f64| <= (k - 1) 2^-24 sum_j |table[gather_j]| per element: k - 1 additions, each rounded
    once by at most 2^-24 of a partial sum that the sum of magnitudes bounds (derived, not measured)."""
    src, blocks, n, table_rows = apc.form_case_senders(k, seed=k)
    gen = torch.Generator().manual_seed(100 + k)
    table = torch.randn(table_rows, 64, generator=gen)
    table[::7] *= 1000.0                                                      # cancellation between large rows
    got = apc.sum_kernel_order(table, src, n, k)
    want = apc.sum_f64(table, src, n, k)
    bound = apc.sum_bound(table, src, n, k)
    assert got.dtype == torch.float32 and want.dtype == torch.float64 and got.shape == want.shape == (n, 64)
    assert bool(((got.double() - want).abs() <= bound).all())
    if k == 1:
        assert torch.equal(got, table[src.long()])
    # the order is the kernel's: a balanced tree for 8 / 16, left to right from +0.0 otherwise
    rows = torch.zeros(1, k, 1)
    rows[0, :, 0] = torch.tensor([2.0 ** 24] + [1.0] * (k - 1))
    tree = {8: 2.0 ** 24 + 6.0, 16: 2.0 ** 24 + 14.0}                         # 2^24 + 1 rounds to 2^24; pairs of ones survive
    assert float(apc.sum_rows_kernel_order(rows)) == tree.get(k, 2.0 ** 24)
    zeros = apc.sum_rows_kernel_order(torch.full((1, k, 4), -0.0))
    assert bool((torch.signbit(zeros) == (k in (8, 16))).all())               # 0.0 + -0.0 = +0.0; -0.0 + -0.0 = -0.0


def test_same_bits_compares_bits_and_nan_positions():
    a = torch.tensor([0.0, 1.0, float("nan"), float("inf")])
    assert apc.same_bits(a, a.clone())
    assert not apc.same_bits(a, torch.tensor([-0.0, 1.0, float("nan"), float("inf")]))
    assert not apc.same_bits(a, torch.tensor([0.0, float("nan"), float("nan"), float("inf")]))
    assert not apc.same_bits(a, torch.tensor([0.0, 1.0, 2.0, float("inf")]))
    other_nan = a.clone()
    other_nan.view(torch.int32)[2] = 0x7FC00001                               # another payload: still "NaN here"
    assert apc.same_bits(a, other_nan)


# ---- cgnn_aggregate_planned_form: no allocation, no device ----------------------------------------------------------

def _form(table_rows, num_nodes, k, width):
    return _lib.load().cgnn_aggregate_planned_form(table_rows, num_nodes, k, width)


@pytest.mark.parametrize("width,table_rows,sl", [(128, 8388605, 4), (128, 8388606, 0), (256, 4194302, 8), (256, 4194303, 0),
                                                 (128, 0, 0), (256, 0, 0), (128, 1, 4), (256, 1, 8)])
def test_form_on_each_side_of_the_4_gib_limit(width, table_rows, sl):
    for k, kk in ((16, 16), (8, 8), (5, 0)):
        assert _form(table_rows, 8192, k, width) == kk * 16 + sl
    # the limit is NO_ROW itself, and the receivers count as rows of the (output) table
    assert (table_rows * width * 4 <= apc.NO_ROW) == (sl != 0) or table_rows == 0
    if sl:
        assert _form(table_rows, table_rows, 16, width) == 16 * 16 + sl
        assert _form(1, apc.NO_ROW // (width * 4) + 1, 16, width) == 16 * 16


@pytest.mark.parametrize("width", [64, 32, 96, 160, 224, 288, 512])
@pytest.mark.parametrize("table_rows", [0, 1, 9000, 8388605, 1 << 40])
def test_other_widths_take_the_general_slice_loop(width, table_rows):
    for k, kk in ((16, 16), (8, 8), (11, 0)):
        assert _form(table_rows, 9000, k, width) == kk * 16


@pytest.mark.parametrize("k,kk", [(8, 8), (16, 16), (1, 0), (5, 0), (11, 0), (12, 0), (32, 0), (7, 0), (9, 0), (15, 0),
                                  (17, 0)])
def test_form_of_each_k(k, kk):
    assert _form(9000, 9000, k, 128) == kk * 16 + 4
    assert _form(9000, 9000, k, 256) == kk * 16 + 8
    assert _form(0, 9000, k, 128) == _form(9000, 9000, k, 64) == kk * 16
    assert _form(9000, 0, k, 128) == kk * 16 + 4                              # no receivers: still a valid call


def test_form_refusals_are_the_launchers():
    lib = _lib.load()
    assert _form(9000, 9000, 33, 128) == apc.ERR_UNSUPPORTED and b"fixed_k" in lib.cgnn_last_error()
    assert _form(9000, 9000, 16, 48) == apc.ERR_UNSUPPORTED
    assert _form(9000, 9000, 16, 130) == apc.ERR_UNSUPPORTED
    for args in ((9000, 9000, 0, 128), (9000, 9000, -1, 128), (9000, 9000, 16, 0), (9000, 9000, 16, -32),
                 (-1, 9000, 16, 128), (9000, -1, 16, 128)):
        assert _form(*args) == apc.ERR_INVALID_ARG
    # the launcher refuses the same calls with the same status before it touches a pointer (none below is dereferenced)
    fake = 1 << 20
    for args, rc in (((9000, 33, 128), apc.ERR_UNSUPPORTED), ((9000, 16, 48), apc.ERR_UNSUPPORTED),
                     ((9000, 0, 128), apc.ERR_INVALID_ARG), ((-1, 16, 128), apc.ERR_INVALID_ARG)):
        assert lib.cgnn_aggregate_planned_rows(fake, 9000, fake, fake, *args, fake, None) == rc
        assert lib.cgnn_aggregate_planned(fake, fake, fake, *args, fake, None) == rc
    assert lib.cgnn_aggregate_planned_rows(None, 9000, fake, fake, 9000, 16, 128, fake, None) == apc.ERR_INVALID_ARG
    assert lib.cgnn_aggregate_planned_rows(fake, 9000, fake, fake, 0, 16, 128, fake, None) == 0      # nothing to do


def test_every_case_of_the_gpu_tests_names_its_form():
    for k, width, route, form in apc.FORM_CASES:
        _, n, table_rows = apc.form_case_layout(k, seed=k)
        assert _form(table_rows if route == "rows" else 0, n, k, width) == form, (k, width, route)
    assert _form(apc.EDGE_4G["rows_32bit"], 8192, 16, 128) == 16 * 16 + 4
    assert _form(apc.EDGE_4G["rows_64bit"], 8192, 16, 128) == 16 * 16


def test_new_entry_is_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes and name in design
    # next to the planned entries in the header, and one definition that the launcher calls
    assert header.index("cgnn_aggregate_planned_rows(") < header.index("cgnn_aggregate_planned_form(") < header.index("K8+K9")
    source = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "aggregate_plan.hip")).read()
    launcher = source[source.index("int cgnn_aggregate_planned_rows("):]
    assert "cgnn_aggregate_planned_form(table_rows, num_nodes, fixed_k, width)" in launcher
    assert "width == 128" not in launcher and "fixed_k == 16" not in launcher     # no second place that decides
    assert "tests/test_gpu_aggregate_plan_forms.py" in design
