"""CPU, every run: the gates of tests/backward_checks.py tested on themselves, the fragile-row helper, and the tile map
that every persistent kernel shares (``tile_range()`` / ``grid_for_tiles``) restated and checked exhaustively.

The stand-in for a backward kernel is torch's float32 backward on the CPU.  It must pass every gate; a ``du`` with a tile
of the tile loop's second pass replaced by its neighbour, with zero rows wherever ``dy`` is small, with the ReLU mask of
the row 32 above (a stale tile) on those rows, or with LayerNorm's m2 term dropped there must be rejected by the per-row
gate -- while the project's earlier gate, ``max |err| <= 2e-5 max |want|`` over the whole tensor, lets the last three pass
on every row below 5e-6 of the largest (and sees them only by a factor of 1.04 .. 6 on rows up to 1e-4), which is why the
per-row gate exists.  The sizes are those of a made-up device with 4 (or 2) compute units, so that
``rows_past_one_pass`` -- every wave runs two tiles, some three, ragged last tile -- is 2215 (1191) rows; the rows are
margin-filtered (backward_checks.py: a ReLU input at rounding distance from zero makes ANY f32 gradient of its row
discontinuous) and nothing is excluded from a gate."""
import pytest
import torch

import backward_checks as bc
import edge_checks as ec

CUS = 4
SHAPE = (128, 128, 128, 128, 2, True)          # the node model


def _manual_du(p, mask_shift=0, drop_m2=False):
    """The float32 backward of bc.mlp_problem written out as the kernels evaluate it (recompute, LayerNorm through m1 / m2,
    masks from the activations): -> du.  ``mask_shift``: every ReLU mask is taken from the row that many rows above;
    ``drop_m2``: LayerNorm's backward without its zhat * mean(g zhat) term."""
    sd, nh = p["sd"], p["nh"]
    h, masks = p["u"], []
    for i in range(nh):
        a = h @ sd[f"m.0.{2 * i}.weight"].t() + sd[f"m.0.{2 * i}.bias"]
        masks.append(torch.roll(a > 0, mask_shift, 0))
        h = a.relu()
    out = h @ sd[f"m.0.{2 * nh}.weight"].t() + sd[f"m.0.{2 * nh}.bias"]
    g = p["dy"]
    if p["ln"]:
        mean = out.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((out - mean) ** 2).mean(1, keepdim=True) + 1e-5)
        z = (out - mean) * rstd
        gz = g * sd["m.1.weight"]
        m1, m2 = gz.mean(1, keepdim=True), (gz * z).mean(1, keepdim=True)
        g = rstd * (gz - m1 - (0 if drop_m2 else z * m2))
    for l in range(nh, 0, -1):
        g = (g @ sd[f"m.0.{2 * l}.weight"]) * masks[l - 1]
    return g @ sd["m.0.0.weight"]


@pytest.fixture(scope="module")
def case():
    n = bc.rows_past_one_pass(2, CUS)
    p, want, yard = bc.mlp_case(11, n, *SHAPE)
    stand_in = bc.mlp_reference(p, torch.float32)
    return p, want, yard, stand_in


def test_the_float32_stand_in_passes_every_gate(case):
    p, want, yard, y = case
    fin = p["fin"]
    st = bc.check_mlp(p, want, y["du"][:, :fin], y["du"][:, fin:], y["grads"], "stand-in")
    bc.report("cpu stand-in node model", st, yard)
    assert st["row"] <= 0.25 * bc.GTOL and st["param"] <= 0.25 * bc.GTOL          # the yardstick's quarter
    # the same backward written out by hand (what the mutations below are made from) is as good
    assert bc.assert_rows(_manual_du(p), want["du"], "manual du") <= 0.25 * bc.GTOL
    # the edge round's gates on its float32 stand-in (1191 edges rounded down to k = 8 on a made-up device with 2 CUs)
    ne = bc.rows_past_one_pass(2, 2)
    pe, wante, yarde = bc.edge_case(5, 64, 64, 2, "k8", ne // 8)
    bc.assert_runs_passes(pe["ne"], 2, 2)
    st = bc.check_edge(pe, wante, bc.edge_reference(pe, torch.float32), "edge stand-in")
    bc.report("cpu stand-in edge round", st, yarde)


def _old_gate(du, want):
    return bc.max_norm_err(du, want["du"]) <= bc.GTOL


def test_a_wrong_tile_in_the_second_pass_is_rejected(case):
    p, want, _, y = case
    du = y["du"].clone()
    tile = bc.second_pass_tile(p["n"], CUS)
    assert tile == bc.grid_for_tiles((p["n"] + 31) // 32, CUS) // 8 * 4 and (tile + 1) * 32 <= p["n"]      # wave 0's second tile
    with ec.corrupted_tile(du, tile):
        ec.must_fail(bc.assert_rows, du, want["du"], "du")
    assert bc.assert_rows(du, want["du"], "du") <= 0.25 * bc.GTOL                # restored
    # the last, ragged tile as well
    with ec.corrupted_tile(du, (p["n"] - 1) // 32):
        ec.must_fail(bc.assert_rows, du, want["du"], "du")


@pytest.mark.parametrize("mutation", ["zero", "stale mask", "m2 dropped"])
def test_what_the_whole_tensor_gate_cannot_see_is_rejected_per_row(case, mutation):
    """Rows whose dy factor is below 1e-4 (half of them) are wrong: zero, computed with the ReLU masks of the row 32 above,
    or without LayerNorm's m2 term.  The per-row gate rejects each.  The whole-tensor 2e-5 gate sees an error of the size
    of a row only down to rows of 2e-5 of the largest: with all rows below 1e-4 wrong it measures 1.2e-4 (zero), 1.1e-4
    (stale mask) and 2.1e-5 (m2 dropped: the term is 1 / sqrt(D) of the row), so it still notices -- by a factor of 6 to
    1.04, where the per-row gate has 2e4.  The same three mutations on the rows below 5e-6 (a subset, 30 % of all rows)
    pass it outright and are rejected per row all the same: that is the reason for the per-row gate."""
    p, want, _, y = case
    wrong = {"zero": lambda: torch.zeros_like(y["du"]), "stale mask": lambda: _manual_du(p, mask_shift=32),
             "m2 dropped": lambda: _manual_du(p, drop_m2=True)}[mutation]()
    small = p["dy_scale"] < 1e-4
    assert 0.4 * p["n"] < int(small.sum()) < 0.6 * p["n"]
    du = torch.where(small[:, None], wrong, y["du"])
    ec.must_fail(bc.assert_rows, du, want["du"], "du")
    worst, where = bc.row_err(du, want["du"])
    assert bool(small[where]) and worst > 1e-2, (mutation, worst)               # O(1) of the row, 500 x the gate
    old = bc.max_norm_err(du, want["du"])
    print(f"{mutation}: rows with dy below 1e-4 -> worst row {worst:.2e}, whole-tensor max-norm {old:.2e}")
    tiny = p["dy_scale"] < 5e-6
    assert int(tiny.sum()) > 0.25 * p["n"]
    du = torch.where(tiny[:, None], wrong, y["du"])
    assert _old_gate(du, want), bc.max_norm_err(du, want["du"])
    ec.must_fail(bc.assert_rows, du, want["du"], "du")


def test_fragile_rows_are_redrawn_deterministically_and_within_the_cap():
    n = 6000
    p = bc.mlp_problem(3, n, *SHAPE)
    assert 0 < p["redrawn"] <= bc.REDRAW_CAP * n                                  # about 0.5 % at 128 -> 128 -> 128 -> 128
    assert not bool(bc.fragile_rows(bc.mlp_pre_activations(p["sd"], p["u"], p["nh"])).any())
    q = bc.mlp_problem(3, n, *SHAPE)
    assert q["redrawn"] == p["redrawn"] and torch.equal(q["u"], p["u"]) and torch.equal(q["dy"], p["dy"])
    assert not torch.equal(bc.mlp_problem(4, n, *SHAPE)["u"], p["u"])
    # the helper finds a planted row, re-draws only that one, and the cap is an assertion
    gen = torch.Generator().manual_seed(0)
    u = p["u"].clone()
    a = bc.mlp_pre_activations(p["sd"], u[77:78], 1)[0][0]
    w0 = p["sd"]["m.0.0.weight"].double()
    u[77] = (u[77].double() - a[5] * w0[5] / (w0[5] @ w0[5])).float()             # hidden unit 5 of row 77 lands on zero
    assert bool(bc.fragile_rows(bc.mlp_pre_activations(p["sd"], u, p["nh"]))[77])
    before = u.clone()
    assert bc.redraw_fragile_mlp_rows(gen, p["sd"], u, p["nh"]) == 1
    changed = (u != before).any(dim=1)
    assert int(changed.sum()) == 1 and bool(changed[77])
    with pytest.raises(AssertionError, match="re-drawn"):
        bc.redraw_fragile_mlp_rows(gen, p["sd"], before, p["nh"], cap=1e-5)
    # edge problems: the e row is what gets re-drawn
    pe = bc.edge_problem(9, 128, 128, 2, "k16", 400)
    assert 0 < pe["redrawn"] <= bc.REDRAW_CAP * pe["ne"]
    assert not bool(bc.fragile_rows(bc.edge_pre_activations(pe["sd"], pe["x"], pe["src"], pe["dst"], pe["e"], 2, 128)).any())
    assert torch.equal(bc.edge_problem(9, 128, 128, 2, "k16", 400)["e"], pe["e"])


def test_row_counts_run_every_wave_twice():
    for cus in (2, 4, 64, 256, 304):
        for passes in (1, 2, 3):
            n = bc.rows_past_one_pass(passes, cus)
            assert n == 32 * (8 * cus * passes + 5) + 7
            lo, hi = bc.tiles_per_wave(n, cus)
            assert (lo, hi) == (passes, passes + 1)
    assert bc.rows_past_one_pass(2, 256) == 131239
    with pytest.raises(AssertionError):
        bc.assert_runs_passes(65536, 2, 256)                                      # exactly one tile per wave
    with pytest.raises(AssertionError):
        bc.assert_runs_passes(4100, 2, 256)


def _assert_partition(tiles, nb, waves):
    seen = [0] * tiles
    for b in range(nb):
        for w in range(waves):
            for t in bc.tile_range(tiles, nb, b, w, waves):
                assert 0 <= t < tiles, (tiles, nb, waves, b, w, t)
                seen[t] += 1
    assert all(c == 1 for c in seen), (tiles, nb, waves)


def test_tile_range_visits_every_tile_exactly_once():
    """csrc/cgnn_common.hpp tile_range(), restated in backward_checks.tile_range: over grids of 1 .. 24 workgroups and
    8 j up to 512, 1 / 4 / 8 waves per workgroup and 0 .. 300 tiles plus counts around 8 CUs passes, the waves' ranges are
    disjoint and cover [0, tiles)."""
    grids = list(range(1, 25)) + [8 * j for j in range(4, 65)]
    for waves in (1, 4, 8):
        for nb in grids:
            step = 1 if nb <= 24 else 7
            for tiles in list(range(0, 301, step)) + [300]:
                _assert_partition(tiles, nb, waves)
    for cus in (256, 304):
        for passes in (1, 2, 3):
            for d in (-1, 0, 1, 6, 9):
                tiles = 8 * cus * passes + d
                _assert_partition(tiles, bc.grid_for_tiles(tiles, cus), 4)
    # grid_for_tiles: capped at 2 workgroups per CU, a multiple of 8 from 8 on (the XCD-aware branch)
    assert bc.grid_for_tiles(1, 256) == 1 and bc.grid_for_tiles(29, 256) == 8 and bc.grid_for_tiles(10 ** 6, 256) == 512
    assert bc.grid_for_tiles(0, 256) == 1 and bc.grid_for_tiles(4101, 256) == 512
