"""CPU, every run: the geometry, gates and guards of tests/forward_checks.py tested on themselves.

The stand-in for a forward kernel is the float32 yardstick (the operation in torch float32 on the CPU).  It must pass every
gate; the same result with ONE row of 100,519 wrong -- swapped with the row one grid stride of tiles further on, computed
without the output layer's bias, without LayerNorm's beta, without the residual, with activations of one fp16 term, or left at
the previous call's values -- must be rejected by the per-row gate, an overwritten canary by the footprint check, and a read
one row or one column outside a guarded input must surface as NaN.  The 100,519 rows are ``rows_past_one_pass`` of the 32-row
kernels on a made-up device with 196 compute units."""
import pytest
import torch

import backward_checks as bc
import edge_checks as ec
import forward_checks as fc

CUS = 196


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def _brute_force(n, launch, cus):
    """The launch for ``n`` rows played through: which wave visits which tile in which trip of its loop (cgnn_common.hpp
    tile_range() with the launcher's grid).  -> trips[tile]."""
    rows, bpc, waves = fc.LAUNCHES[launch]
    tiles = (n + rows - 1) // rows
    nb = fc.grid_for_tiles(tiles, cus, bpc, waves)
    trips = [None] * tiles
    for b in range(nb):
        for w in range(waves):
            for trip, t in enumerate(fc.tile_range(tiles, nb, b, w, waves)):
                assert trips[t] is None, (n, launch, cus, t)
                trips[t] = trip
    assert all(t is not None for t in trips), (n, launch, cus)
    return trips


@pytest.mark.parametrize("launch", sorted(fc.LAUNCHES))
def test_second_pass_is_what_the_tile_loop_does(launch):
    """Over small devices and every tile count up to three sweeps: a tile is reached in a wave's second trip exactly when the
    restatement says so, ``assert_runs_passes`` accepts a size only if every wave makes a second trip, and the size
    ``rows_past_one_pass`` names has second-pass and third-pass tiles, uneven eighths and a ragged end."""
    rows, bpc, waves = fc.LAUNCHES[launch]
    for cus in (8, 16, 24, 40):
        full = waves * fc.grid_for_tiles(1 << 40, cus, bpc, waves)          # tiles of one sweep of the whole grid
        for tiles in range(1, 3 * full + 12):
            n = tiles * rows - 5
            trips = _brute_force(n, launch, cus)
            _, counts = fc.wave_tile_counts(n, launch, cus)
            assert sum(counts) == tiles and max(counts) == max(trips) + 1
            every_wave_twice = min(counts) >= 2
            try:
                fc.assert_runs_passes(n, launch, 2, cus)
                accepted = True
            except AssertionError:
                accepted = False
            assert not accepted or (every_wave_twice and max(counts) > min(counts) and tiles % 8), (n, launch, cus)
            if tiles <= full:
                assert max(trips) == 0 and not accepted                    # one tile per wave at most: what the suite ran so far
        for passes in (1, 2, 3):
            n = fc.past_one_pass(launch, passes, cus)
            assert n == rows * (full * passes + 5) + 7
            _, counts = fc.wave_tile_counts(n, launch, cus)
            assert (min(counts), max(counts)) == (passes, passes + 1)
            trips = _brute_force(n, launch, cus)
            assert trips.count(passes) >= 1 and trips.count(passes - 1) >= full - 8


def test_rows_past_one_pass_on_real_devices():
    want = {8: (4263, 2135, 2215), 104: (53415, 26711, 26791), 256: (131239, 65623, 65703), 304: (155815, 77911, 77991)}
    for cus, (two_per_cu, n16, one_per_cu) in want.items():
        assert fc.rows_past_one_pass(32, 2, 4, cus=cus) == two_per_cu == bc.rows_past_one_pass(2, cus)
        assert fc.rows_past_one_pass(16, 1, 8, cus=cus) == n16
        assert fc.rows_past_one_pass(32, 1, 4, cus=cus) == one_per_cu == fc.past_one_pass("node_x3", 2, cus)
        n = fc.ring_rows_past_one_pass(2, cus)
        assert n == 128 * (2 * cus + 5) + 7 == fc.ring_rows_past_one_pass(2, cus, edge=True)
    with pytest.raises(AssertionError):
        fc.assert_runs_passes(65536, "rows32", 2, 256)                      # exactly one tile per wave
    with pytest.raises(AssertionError):
        fc.assert_runs_passes(6000, "rows32", 2, 256)                       # the largest direct call of the suite so far
    assert fc.project_launch("fp16x2", 128, 128, 4096) == "rows32_lds" and fc.project_launch("fp16x2", 128, 128, 4095) == "rows32"
    assert fc.project_launch("fp16x2", 64, 128, 5000) == "rows32" and fc.project_launch("fp32", 128, 128, 5000) == "rows32"


def test_ring_step_loops_visit_every_step_once():
    for cus in (7, 8, 256):
        for n in list(range(1, 128 * (3 * cus + 2), 61 if cus < 256 else 4099)):
            steps, grid, per = fc.ring_steps(n, cus)
            seen = sorted(s for b in range(grid) for s in range(b, steps, grid))
            assert seen == list(range(steps)) and sum(per) == steps and grid == min(steps, cus)
            full, egrid, eper, ragged = fc.edge_ring_steps(n, cus)
            assert 128 * full + 16 * ragged == 32 * ((n + 31) // 32) and sum(eper) == full and ragged in (0, 2, 4, 6)
        n = fc.ring_rows_past_one_pass(2, cus)
        assert sorted(set(fc.ring_steps(n, cus)[2])) == [2, 3] and n % 128 == 7
        assert sorted(set(fc.edge_ring_steps(n, cus)[2])) == [2, 3]


# ---- gates ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def node():
    n = fc.past_one_pass("rows32", 2, CUS)
    assert n == 100519
    case = fc.node_case(7, n, 32, 32, 1)
    stand_in = fc.forward(case[0], torch.float32)
    return case, stand_in


def test_the_yardstick_meets_a_quarter_of_the_cap(node):
    cases = {"node": node[0], "encoder": fc.mlp_case(1, 3000, 17, 64, 64, 2, True), "decoder": fc.mlp_case(2, 3000, 64, 64, 3, 2, False),
             "edge": fc.edge_case(3, 3003, 700, 64, 128, 2), "edge k8": fc.edge_case(4, 2400, 300, 32, 32, 1, "k8"),
             "projection": fc.projection_case(5, 3000, 64, 128)}
    for what, (p, want, yard, G) in cases.items():
        for k in want:
            assert 0 < yard[k] <= 0.25 * fc.G_CAP and G[k] == 4 * yard[k], (what, k, yard[k])
            print(f"cpu yardstick {what} {k}: worst row {yard[k]:.2e}, G {G[k]:.2e}")
    stand_in = {k: v for k, v in node[1].items()}
    fc.check(node[0], stand_in, "cpu stand-in node (32,32)")
    p = cases["edge"][0]
    assert int(p["src"].min()) == int(p["dst"].min()) == 0 and int(p["src"].max()) == int(p["dst"].max()) == p["nodes"] - 1
    # a problem whose own float32 evaluation is bad is refused, not given a looser gate
    with pytest.raises(AssertionError, match="cap"):
        fc.gate_from_yardstick(3e-6, "degenerate")


@pytest.mark.parametrize("defect", ["swapped", "stale"] + list(fc.DEFECTS))
def test_one_wrong_row_in_a_hundred_thousand_is_rejected(node, defect):
    (p, want, yard, G), stand_in = node
    n = p["n"]
    row, stride = fc.second_pass_row(n, "rows32", CUS)
    assert row >= 200 and row + stride < n and stride == 32 * 4 * (2 * CUS // 8)
    for name in ("x_out", "u"):
        if name == "u" and defect == "residual missing":
            continue
        got = stand_in[name].clone()
        if defect == "swapped":                   # the values of the tile one grid stride on: a wrong tile index
            got[row] = stand_in[name][row + stride]
        elif defect == "stale":                   # the row was never written: it holds the previous call's result
            got[row] = fc.forward(fc.node_problem(8, 256, 32, 32, 1), torch.float32)[name][row % 256]
        else:
            got[row] = fc.forward(p, torch.float32, rows=slice(row, row + 1), defect=defect)[name][0]
        worst, where = fc.row_err(got, want[name])
        print(f"{defect} {name}: row {row} off by {worst:.2e} of its norm (G {G[name]:.2e}), whole-tensor "
              f"max-norm {fc.tensor_err(got, want[name]):.2e} (contract {fc.TENSOR_TOL:.0e})")
        assert where == row and worst > 4 * G[name], (defect, name, worst)
        ec.must_fail(fc.assert_rows, got, want[name], G[name], defect)
        got[row] = stand_in[name][row]
        fc.assert_rows(got, want[name], G[name], "restored")
    if defect == "one fp16 term":
        # why the gate is per row: the tensor contract alone lets this defect through, even on EVERY row of the 1e-3 block
        got = stand_in["x_out"].clone()
        got[60:110] = fc.forward(p, torch.float32, rows=slice(60, 110), defect=defect)["x_out"]
        assert fc.tensor_err(got, want["x_out"]) <= fc.TENSOR_TOL
        ec.must_fail(fc.assert_rows, got, want["x_out"], G["x_out"], defect)


def test_the_residual_gate_is_element_wise():
    p, want, _, _ = fc.edge_case(3, 3003, 700, 64, 128, 2)
    y = fc.forward(p, torch.float32)
    fc.assert_residual_sum(y["e_out"], p["e"], y["u"], "stand-in")
    bad = y["e_out"].clone()
    bad[2999, 5] = y["u"][2999, 5]
    ec.must_fail(fc.assert_residual_sum, bad, p["e"], y["u"], "residual missing in one element")
    bad = y["e_out"].clone()
    bad[70, 9] += 2.0 ** -20 * abs(float(y["u"][70, 9]))            # four units of the last place of u, in the 1e-3 block
    ec.must_fail(fc.assert_residual_sum, bad, p["e"], y["u"], "four ulps")


# ---- guards -----------------------------------------------------------------------------------------------------------------
def test_an_overwritten_canary_is_rejected():
    n, w = 77, 3
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        buf, view = fc.canary_output(n, w, "cpu", ld=8, rows_before=5, dtype=dtype)
        assert view.shape == (n, w) and view.stride(0) == 8 and buf.shape[0] == 5 + n + fc.SPARE_ROWS
        fc.assert_canaries(buf, (5, 5 + n), w, "untouched")
        view.copy_(torch.randn(n, w).to(dtype))
        fc.assert_canaries(buf, (5, 5 + n), w, "written")
        for r, c, what in ((5 + n, 0, "row n"), (4, 2, "the row before"), (5 + n - 1, w, "the column behind the last row"),
                           (buf.shape[0] - 1, 7, "the last cell")):
            saved = buf[r, c].clone()
            buf[r, c] = 1.0
            with pytest.raises(AssertionError, match="canary"):
                fc.assert_canaries(buf, (5, 5 + n), w, what)
            buf[r, c] = saved
            fc.assert_canaries(buf, (5, 5 + n), w, "restored")
        buf[5 + n, 1] = 0.0                                   # a zero is a write too
        ec.must_fail(fc.assert_canaries, buf, (5, 5 + n), w, "zero at row n")
    # TILED32 outputs: rows n .. cgnn_tiled_rows(n) are scratch, everything behind is canary
    buf, view = fc.canary_output(96, 32, "cpu")
    buf[70:96] = 3.0
    fc.assert_canaries(buf, (0, 96), 32, "scratch rows")
    buf[96, 0] = 3.0
    ec.must_fail(fc.assert_canaries, buf, (0, 96), 32, "behind the tiles")


def test_a_read_outside_a_guarded_input_is_seen():
    p, want, _, G = fc.mlp_case(1, 3000, 17, 64, 64, 2, True)
    n, d = p["x"].shape
    x = fc.guarded(p["x"], "cpu", ld=20)
    assert x.shape == (n, d) and x.stride() == (20, 1) and torch.equal(x, p["x"]) and x.data_ptr() % 16 == 0
    fc.assert_rows(fc.forward(dict(p, x=x), torch.float32)["y"], want["y"], G["y"], "inside")
    one_row_late = torch.as_strided(x, (n, d), (20, 1), x.storage_offset() + 20)              # reads row n
    one_row_early = torch.as_strided(x, (n, d), (20, 1), x.storage_offset() - 20)             # reads row -1
    one_column_wide = torch.as_strided(x, (n, d + 1), (20, 1), x.storage_offset())             # reads column d with weight 0
    for what, xs in (("row n", one_row_late), ("row -1", one_row_early)):
        with pytest.raises(AssertionError, match="non-finite"):
            fc.assert_rows(fc.forward(dict(p, x=xs), torch.float32)["y"], want["y"], G["y"], what)
    w0, b0 = p["lins"][0]
    wide = dict(p, x=one_column_wide, lins=[(torch.cat([w0, torch.zeros(w0.shape[0], 1)], dim=1), b0)] + p["lins"][1:])
    with pytest.raises(AssertionError, match="non-finite"):
        fc.assert_rows(fc.forward(wide, torch.float32)["y"], want["y"], G["y"], "column d")
    # index arrays are surrounded by -1, which addresses the NaN row in front of a guarded table
    src = fc.guarded(torch.arange(5, dtype=torch.int32).view(-1, 1), "cpu").reshape(-1)
    table = fc.guarded(torch.ones(5, 4), "cpu")
    late = torch.as_strided(src, (5,), (1,), src.storage_offset() + 1)
    gathered = torch.as_strided(table, (6, 4), (4, 1), table.storage_offset() - 4)[late.long() + 1]
    assert torch.equal(src, torch.arange(5, dtype=torch.int32)) and int(late[-1]) == -1 and bool(torch.isnan(gathered[-1]).all())
