"""CPU, every run: the row partitions of the parameter-gradient reductions restated in tests/reduction_checks.py against the
library's own workspace sizes (the library loads without a GPU), their coverage of [0, n), the branch finders pinned to the
numbers the kernels' code implies, and the exact gate tested on itself: float32 stand-ins that follow the partitions pass
``assert_exact``, and every planted defect -- a dropped last partial step, a partial taken twice, a stale workspace slot, a row
beyond n, a skipped input tile of a partial group, a write to column col0 - 1, each of the six bf16 products removed -- is
rejected."""
import pytest
import torch

import reduction_checks as rc
from cosmology_gnn_simulation_amd import _lib


# ---- partitions --------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (3, 128), (128, 17), (33, 97), (128, 128), (128, 256), (160, 224), (256, 256), (512, 512), (1024, 256))
ROWS = (1, 7, 8, 9, 1023, 1024, 1025, 2049, 7169, 8193, 65537, 262144, 262145, 262153, 300000, 1 << 20, 5_000_000)


def test_restated_workspace_sizes_match_the_library():
    lib = _lib.load()
    for (o, i), n in ((s, n) for s in SHAPES for n in ROWS):
        assert rc.wgrad_workspace_bytes(n, o, i) == lib.cgnn_weight_grad_workspace_bytes(n, o, i), (n, o, i)
    for n in ROWS:
        for width in (1, 3, 4, 5, 20, 64, 128, 252, 256, 260, 516):
            assert rc.col_dot_workspace_bytes(n, width) == lib.cgnn_col_dot_workspace_bytes(n, width), (n, width)
    assert lib.cgnn_weight_grad_x3_workspace_bytes() == rc.X3_PARTS * rc.X3_PART_FLOATS * 4
    assert lib.cgnn_weight_grad_workspace_bytes(0, 128, 128) == 0 and lib.cgnn_col_dot_workspace_bytes(0, 4) == 0
    # the sweep crosses the cap: capped and uncapped shapes on both sides
    assert any(rc.wgrad_ordered_shape(n, o, i)[1] > rc.WGRAD_ROWS for (o, i) in SHAPES for n in ROWS)
    assert any(rc.wgrad_cap(o, i) > rc.WGRAD_MAX_CHUNKS for (o, i) in SHAPES)


NAMED = (16401, 16384, 16385, 262145, 262153, 32 * 1024 + 16 * 3 + 5, 9 * 512 - 1)


def test_partitions_cover_every_row_once():
    for n in list(range(1, 2100)) + list(NAMED):
        shapes = ((3, 128), (256, 256)) if n < 2100 else ((256, 256),)
        for o, i in shapes:
            chunks, rows, po, pi = rc.wgrad_ordered_shape(n, o, i)
            assert rows % 8 == 0 and chunks >= 1 and (chunks - 1) * rows < n <= chunks * rows, (n, o, i)
            assert rc.covers_once(rc.wgrad_chunks(n, o, i, "ordered"), n) and len(rc.wgrad_chunks(n, o, i, "ordered")) == chunks
            assert rc.covers_once(rc.wgrad_chunks(n, o, i, "atomic"), n)
        p = rc.x3_partition(n)
        waves = rc.x3_wave_rows(n)
        assert len(waves) == rc.X3_WAVES and rc.covers_once(waves, n)
        assert p["rows_per_wave"] % 16 == 0 and p["live"] + p["idle"] == rc.X3_WAVES
        assert sum(1 for r0, r1 in waves if r0 < r1) == p["live"]
        assert waves[p["live"] - 1][1] - waves[p["live"] - 1][0] == p["last_rows"] == 16 * p["last_full"] + p["last_tail"]
        steps = rc.x3_wave_steps(n)
        assert steps[p["live"] - 1] == (p["last_full"], p["last_tail"]) and sum(16 * f + t for f, t in steps) == n
        assert all(s == (p["rows_per_wave"] // 16, 0) for s in steps[:p["live"] - 1]) and all(s == (0, 0) for s in steps[p["live"]:])
        assert rc.covers_once(rc.col_dot_shape(n, 4)[0], n) and rc.covers_once(rc.colsum_blocks(n), n)
    for width in range(1, 600):
        _, passes = rc.col_dot_shape(1, width)
        at = 0
        for ps in passes:
            assert ps["c0"] == at and ps["groups"] <= ps["cols"] <= 64 and ps["cols"] * ps["rl"] == rc.BLOCK
            assert ps["cols"] < 2 * ps["groups"] or ps["groups"] == 1
            at += 4 * ps["groups"]
        assert at - 3 <= width <= at and len(passes) == (width + 255) // 256


def test_wave_items_of_the_shapes_the_gpu_file_uses():
    it = rc.wgrad_items
    assert it(128, 17)["G"] == 1 and it(3, 33)["G"] == 2 and it(32, 128)["G"] == 4
    assert [it(1, i)["partial_group"] for i in (64, 96, 128, 160, 224, 256)] == [False, True, False, True, True, False]
    assert (it(96, 17)["n_items"], it(160, 32)["n_items"], it(160, 64)["n_items"], it(256, 256)["n_items"]) == (3, 5, 5, 16)
    assert it(96, 17)["ragged_items"] and it(160, 64)["grid_y"] == 2 and it(96, 96)["n_items"] == 6


# ---- branch finders ----------------------------------------------------------------------------------------------------------
def test_branch_finders_return_what_the_kernels_imply():
    assert rc.x3_smallest_n("full_then_tail") == 16401
    assert rc.x3_partition(16401) == dict(rows_per_wave=32, live=513, idle=511, last_rows=17, last_full=1, last_tail=1)
    assert rc.x3_smallest_n("tail_only") == 1
    assert rc.x3_smallest_n("full_only") == 16384
    assert [rc.x3_way(n) for n in (1, 15, 16, 17, 16383, 16384, 16385, 16401)] == \
        ["tail_only", "tail_only", "full_only", "tail_only", "tail_only", "full_only", "tail_only", "full_then_tail"]
    p = rc.x3_partition(32 * 1024 + 16 * 3 + 5)
    assert (p["rows_per_wave"], p["last_full"], p["last_tail"]) == (48, 2, 5)
    big = rc.x3_smallest_n("full_then_tail", start=300_000, min_full=3)
    p = rc.x3_partition(big)
    assert big == 300_001 and p["last_full"] >= 3 and p["last_tail"] and p["rows_per_wave"] == 304
    assert rc.wgrad_smallest_capped_n(256, 256) == 262145
    assert rc.wgrad_ordered_shape(262153, 256, 256) == (255, 1032, 256, 256)      # fewer chunks than the cap
    assert rc.wgrad_workspace_bytes(262153, 256, 256) == 255 * (256 * 256 + 256) * 4
    assert rc.wgrad_ordered_shape(262144, 256, 256) == (256, 1024, 256, 256)
    assert [rc.wgrad_n_for_chunks(c, 32, 32) for c in (7, 8, 9)] == [6145, 7169, 8193]
    assert rc.wgrad_smallest_capped_n(128, 128) == 1024 * 1024 + 1               # 64 MiB / 64 KiB chunks: out of the tests' reach


# ---- the gate on itself --------------------------------------------------------------------------------------------------------
def test_assert_exact_sees_one_element_and_one_canary_bit():
    want = torch.arange(20.0).view(4, 5)
    block = (slice(1, 3), slice(1, 4))
    rc.assert_exact(want.clone(), want, "same", block)
    got = want.clone()
    got[2, 3] += 1
    with pytest.raises(AssertionError, match=r"1 of 20 elements wrong \(0 canaries\); first at \(2, 3\) \(block\)"):
        rc.assert_exact(got, want, "one", block)
    got = want.clone()
    got[0, 0] = -0.0                                    # equal as a value, not as bits
    with pytest.raises(AssertionError, match=r"first at \(0, 0\) \(CANARY\)"):
        rc.assert_exact(got, want, "canary", block)
    nan = want.clone()
    nan[1, 1] = rc.NAN
    with pytest.raises(AssertionError):
        rc.assert_exact(nan, nan, "NaN in the block is wrong even against itself", block)
    with pytest.raises(AssertionError):
        rc.check_magnitude(1 << 19, 2)
    rc.check_magnitude(262153, 2)


ORDERED_CASES = (          # (n, out_dim, in_dim, col0, ld_g, g_exp, a_exp)
    (2049 + 3, 33, 70, 3, 40, 0, 0),                 # three chunks, G = 2 with a partial last group
    (9, 128, 17, 0, None, -30, 10),
    (rc.wgrad_n_for_chunks(9, 3, 160) + 4, 3, 160, 128, None, 0, 0),     # nine chunks: two trips of reduce lane 0; G = 4, partial
)


def _run(standin, p, calls=2, **kw):
    dw, db = p["dw0"].clone(), p["db0"].clone()
    for _ in range(calls):
        standin(p, dw, db, **kw)
    return dw, db


def _check_wgrad(p, dw, db, calls=2):
    want_dw, want_db = rc.wgrad_expected(p, calls)
    rc.assert_exact(dw, want_dw, "dw", rc.wgrad_block(p))
    rc.assert_exact(db, want_db, "db", p["db_span"])


@pytest.mark.parametrize("case", ORDERED_CASES)
@pytest.mark.parametrize("form", ["ordered", "atomic"])
def test_ordered_stand_in_passes_and_every_planted_defect_is_rejected(case, form):
    n, o, i, col0, ld_g, ge, ae = case
    p = rc.wgrad_problem(5, n, o, i, ld_g=ld_g, col0=col0, g_exp=ge, a_exp=ae)
    _check_wgrad(p, *_run(rc.standin_wgrad, p, form=form))
    # the workspace's contents are irrelevant: the previous call's partials of another problem in it
    chunks, _, po, pi = rc.wgrad_ordered_shape(n, o, i)
    stale = torch.randint(-99, 100, (max(chunks, len(rc.wgrad_chunks(n, o, i, form))), po * pi + po)).float()
    _check_wgrad(p, *_run(rc.standin_wgrad, p, form=form, workspace=stale.clone()))
    defects = ["chunk_twice", "stale_slot", "row_beyond_n"]
    defects += ["drop_last_step"] if n % 8 else []
    defects += ["skip_tile"] if rc.wgrad_items(o, i)["partial_group"] else []
    defects += ["write_col0_minus_1"] if col0 else []
    assert len(defects) >= 4
    for d in defects:
        for fill in (rc.NAN, None):       # a NaN workspace, and one that holds finite stale partials
            ws = stale.clone() if fill is None else torch.full_like(stale, fill)
            with pytest.raises(AssertionError, match="elements wrong"):
                _check_wgrad(p, *_run(rc.standin_wgrad, p, form=form, workspace=ws, defect=d))


def test_all_ordered_defects_are_exercised():
    want = {"chunk_twice", "stale_slot", "row_beyond_n", "drop_last_step", "skip_tile", "write_col0_minus_1"}
    seen = set()
    for n, o, i, col0, *_ in ORDERED_CASES:
        seen |= {"chunk_twice", "stale_slot", "row_beyond_n"} | ({"drop_last_step"} if n % 8 else set())
        seen |= ({"skip_tile"} if rc.wgrad_items(o, i)["partial_group"] else set()) | ({"write_col0_minus_1"} if col0 else set())
    assert seen == want


@pytest.mark.parametrize("n,col0", [(rc.x3_smallest_n("full_then_tail"), 128), (17, 0)])
def test_x3_stand_in_passes_and_every_planted_defect_is_rejected(n, col0):
    p = rc.wgrad_problem(7, n, 128, 128, ld_g=136, ld_a=136, g_col=4, a_col=4, col0=col0, g_exp=-100)
    assert rc.x3_partition(n)["last_tail"] and rc.x3_partition(n)["idle"] >= 4
    _check_wgrad(p, *_run(rc.standin_x3, p))
    stale = torch.randint(-99, 100, (rc.X3_PARTS, 128 * 128 + 128)).float()
    _check_wgrad(p, *_run(rc.standin_x3, p, workspace=stale.clone()))
    for d in ["drop_last_step", "chunk_twice", "stale_slot", "row_beyond_n"] + (["write_col0_minus_1"] if col0 else []):
        for ws in (stale.clone(), torch.full_like(stale, rc.NAN)):
            with pytest.raises(AssertionError, match="elements wrong"):
                _check_wgrad(p, *_run(rc.standin_x3, p, calls=1, workspace=ws, defect=d), calls=1)


@pytest.mark.parametrize("n,width", [(9 * 512 - 1, 20), (513, 260), (257, 5)])
def test_col_dot_stand_in_passes_and_planted_defects_are_rejected(n, width):
    p = rc.col_dot_problem(3, n, width)

    def run(**kw):
        o_ab, o_a = p["out0"].clone(), p["out0"].clone()
        for _ in range(2):
            rc.standin_col_dot(p, o_ab, o_a, **kw)
        rc.assert_exact(o_ab, rc.col_dot_expected(p, "want_ab", 2), "out_ab", p["span"])
        rc.assert_exact(o_a, rc.col_dot_expected(p, "want_a", 2), "out_a", p["span"])

    run()
    stale = torch.randint(-99, 100, (len(rc.col_dot_shape(n, width)[0]), 2, width)).float()
    run(workspace=stale.clone())
    for d in ("chunk_twice", "stale_slot", "row_beyond_n", "write_behind_width"):
        for ws in (stale.clone(), torch.full_like(stale, rc.NAN)):
            with pytest.raises(AssertionError, match="elements wrong"):
                run(workspace=ws, defect=d)


# ---- the three bf16 terms ------------------------------------------------------------------------------------------------------
def test_split_is_greedy_and_exact_on_what_the_probes_hold():
    x = torch.tensor([1 + 2.0 ** -10 + 2.0 ** -20, 3 * (1 + 2.0 ** -10 + 2.0 ** -20), 2 * (1 + 2.0 ** -10), 3.0, -4.0 * 2.0 ** -100])
    x1, x2, x3 = rc.split3(x)
    assert torch.equal(x1, torch.tensor([1.0, 3.0, 2.0, 3.0, -4.0 * 2.0 ** -100]))
    assert torch.equal(x2, torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, 0.0, 0.0]))
    assert torch.equal(x3, torch.tensor([2.0 ** -20, 3 * 2.0 ** -20, 0.0, 0.0, 0.0]))
    gen = torch.Generator().manual_seed(0)
    r = torch.randn(4096, generator=gen) * 10.0 ** torch.randint(-30, 30, (4096,), generator=gen)
    s = rc.split3(r)
    assert float(((s[0].double() + s[1].double() + s[2].double()) - r.double()).abs().div(r.double().abs()).max()) <= 2.0 ** -23


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("name", sorted(rc.PROBES))
def test_each_probe_is_exact_and_needs_its_products(name, n):
    p = rc.probe_problem(name, n)
    g, a = p["g"].values, p["a"].values
    full = rc.x3_product(g, a)
    assert torch.equal(full.double(), p["want"]), "the six products do not give the exact result: a term below them is non-zero"
    # ... and every partial sum that a 16-row step can form is a float32 value.  All rows are the same, so whatever order the
    # matrix core adds the 16 products of one term in, on top of the accumulator c or not, what it holds is k P or c + k P
    acc = torch.zeros(128, 128, dtype=torch.float64)
    gs, as_ = rc.split3(g[:1]), rc.split3(a[:1])
    for tg, ta in rc.X3_TERMS:
        P = gs[tg - 1].double().t() @ as_[ta - 1].double()
        for k in range(1, 17):
            for s in (k * P, acc + k * P):
                assert torch.equal(s.float().double(), s), (name, tg, ta, k)
        acc = acc + 16 * P
    assert torch.equal(acc * (n // 16), p["want"])               # n = 32: two waves of one step each, met in LDS
    for term in rc.X3_TERMS:
        without = rc.x3_product(g, a, tuple(t for t in rc.X3_TERMS if t != term))
        if term in p["needs"]:
            assert not torch.equal(without, full), (name, term)
    dw, _ = rc.standin_x3(p, p["dw0"].clone(), None)
    rc.assert_exact(dw, rc.wgrad_expected(p, 1, with_db=False)[0], name, rc.wgrad_block(p))


def test_every_one_of_the_six_products_has_a_probe_that_rejects_its_removal():
    covered = set()
    for name in rc.PROBES:
        p = rc.probe_problem(name, 16, col0=128)
        want = rc.wgrad_expected(p, 1, with_db=False)[0]
        for term in p["needs"]:
            dw, _ = rc.standin_x3(p, p["dw0"].clone(), None, terms=tuple(t for t in rc.X3_TERMS if t != term))
            with pytest.raises(AssertionError, match="elements wrong"):
                rc.assert_exact(dw, want, f"{name} without {term}", rc.wgrad_block(p))
            covered.add(term)
    assert covered == set(rc.X3_TERMS)


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------
def test_the_per_element_gate_sees_what_the_tensor_norm_does_not():
    """One element of the x 1e-3 column block of the x 1e-8 ... scaled problem computed in half precision: far inside
    max |err| <= 2e-5 max |want|, far outside 4 x the float32 yardstick per element."""
    p = rc.real_problem(1, 128, 128)
    got = p["g"].t() @ p["a"]
    assert rc.elem_ratio(got, p["want"], p["S"]) == p["yard"] <= 2.0 ** -21
    o = 128 // 4 + 1                                     # a column of the x 1e-3 block
    i = int((p["want"][o].abs() / p["S"][o]).argmax())
    got[o, i] = got[o, i].half().float()
    assert float((got.double() - p["want"]).abs().max()) <= 2e-5 * float(p["want"].abs().max())
    assert rc.elem_ratio(got, p["want"], p["S"]) > rc.ARITH_MARGIN * p["yard"]
