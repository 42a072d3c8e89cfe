"""CPU, every run: the migration kernels' geometry restated in tests/migrate_checks.py pinned against include/cgnn.h, csrc/migrate.hip
and ``_lib``; the builders' own properties; the exact problems shown to be exact (a float32 evaluation with one rounding per
operation equals the float64 one); ``ops.group_offsets`` against the definitional prefix; and the exact gate tested on itself:
stand-ins that follow the kernels' lanes, waves and workgroups equal the definitional references on every named pattern at
every size of ``N_EDGES``, and every planted defect -- a lane rank that counts its own lane, a wave sum through the thread's own
wave, the offsets row of the next workgroup, bit 63 dropped, send slots rotated by one, a refused row that takes no place -- is
caught by at least one named pattern."""
import os
import re

import numpy as np
import pytest
import torch

import migrate_checks as mc
from cosmology_gnn_simulation_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_WORLDS = (1, 3, 8, 64)


def _define(text, name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1))


# ---- pinned numbers ----------------------------------------------------------------------------------------------------
def test_geometry_is_the_headers_and_the_librarys():
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    kernel = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "migrate.hip")).read()
    common = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "cgnn_common.hpp")).read()
    assert mc.BLOCK == _define(header, "CGNN_MIGRATE_BLOCK") == _lib.MIGRATE_BLOCK == mc.WAVE * mc.WAVES
    assert "#define CGNN_WAVES_PER_BLOCK (CGNN_BLOCK / CGNN_WAVE)" in common
    assert mc.WAVES == _define(common, "CGNN_BLOCK") // _define(common, "CGNN_WAVE") and mc.WAVE == _define(common, "CGNN_WAVE")
    assert mc.MAX_WORLD == _define(kernel, "CGNN_MIG_MAX_WORLD") == _lib.MIGRATE_MAX_WORLD == 64
    assert mc.MAX_WINDOW == _define(kernel, "CGNN_MIG_MAX_WINDOW") == 32
    assert mc.ROW == _define(header, "CGNN_ROLLOUT_ROW") == _lib.ROLLOUT_ROW
    assert "window in [2, 32], world <= 64" in header
    assert [mc.blocks(n) for n in mc.N_EDGES] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 5] == [ops.migrate_blocks(n) for n in mc.N_EDGES]
    assert mc.blocks(0) == 0
    assert mc.window_lds_bytes(16) == 64 * 1024 and mc.FIRST_WINDOW_ABOVE_64K == 17
    assert mc.window_lds_bytes(mc.MAX_WINDOW) == 128 * 1024
    assert set(mc.WORLDS) <= set(mc.GRIDS) and all(px * py * pz == w for w, (px, py, pz) in mc.GRIDS.items())
    assert {(4, 4, 4), (1, 1, 5), (3, 2, 1), (7, 3, 3)} <= set(mc.GRIDS.values())
    assert max(mc.WORLDS) == mc.MAX_WORLD and mc.FEATURE_WINDOWS == (2, 16, mc.FIRST_WINDOW_ABOVE_64K, mc.MAX_WINDOW)


# ---- builders ------------------------------------------------------------------------------------------------------------
def test_mask_patterns_are_what_their_names_say():
    for world in mc.WORLDS:
        full = (1 << world) - 1
        for n in mc.N_EDGES:
            m = {name: [int(v) for v in mc.mask_pattern(name, n, world)] for name in mc.MASK_PATTERNS}
            assert all(len(v) == n and all(0 <= x <= full for x in v) for v in m.values())
            assert set(m["none"]) == {0} and set(m["all"]) == {full}
            assert set(m["top_bit"]) == {1 << (world - 1)} and set(m["bit_0"]) == {1}
            assert [i for i, x in enumerate(m["lane_0"]) if x] == list(range(0, n, 64))
            assert [i for i, x in enumerate(m["lane_63"]) if x] == list(range(63, n, 64))
            assert [i for i, x in enumerate(m["lanes_alternating"]) if x] == list(range(1, n, 2))
            assert [i for i, x in enumerate(m["empty_wave"]) if not x] == [i for i in range(n) if i // 64 % 4 == 1]
            assert [i for i, x in enumerate(m["last_row"]) if x] == [n - 1]
            assert m["every_group"][n // 2] == full and sum(x != full or world == 1 for x in m["every_group"]) >= n - 1
            on = [i for i, x in enumerate(m["straddle_block"]) if x]
            assert on == [i for i in range(253, 259) if i < n]
            on = [i for i, x in enumerate(m["straddle_wave"]) if x]
            assert on == [i for i in (range(125, 131) if n > 131 else range(61, 67)) if i < n]
    assert int(mc.mask_pattern("all", 3, 64)[0]) == (1 << 64) - 1 and mc.mask_pattern("all", 3, 64).view(np.int64)[0] == -1
    assert mc.mask_pattern("top_bit", 1, 64).view(np.int64)[0] == -2 ** 63           # the sign bit of the int64 mask tensor


def test_destination_patterns_are_what_their_names_say():
    for world in mc.MIGRATE_WORLDS:
        for rank in {0, world - 1}:
            for n in mc.N_EDGES:
                d = {name: mc.dest_pattern(name, n, world, rank) for name in mc.DEST_PATTERNS}
                assert all(v.dtype == np.int32 and v.shape == (n,) for v in d.values())
                assert set(d["all_stay"].tolist()) == {rank} and set(d["all_leave_to_one"].tolist()) == {(rank + 1) % world}
                assert d["round_robin"].tolist() == [i % world for i in range(n)]
                last = (n - 1) // 64 * 64
                stay = d["stayers_in_last_wave"]
                assert set(stay[last:].tolist()) == {rank} and (world == 1 or rank not in stay[:last].tolist())
                bad = d["invalid_sprinkled"]
                for i in range(n):
                    assert (not 0 <= bad[i] < world) == (i % 64 in (0, 63))
                if n >= 257:
                    assert {-1, world, -2 ** 31} <= set(bad.tolist())
                assert int(mc.dest_mask(bad, world)[0]) == 0


def test_layouts_run_every_guard():
    cnt = [5, 0, 7, 9]
    assert mc.halo_layout("packed", cnt)[0].tolist() == [0, 5, 5, 12] and mc.halo_layout("packed", cnt)[1] == 21
    assert mc.halo_layout("short", cnt)[1] == 14 and mc.halo_layout("shifted", cnt)[0].tolist() == [-3, 2, 2, 9]
    starts, cap_out, n_send = mc.migrate_layout("packed", cnt, 2)              # dist.MigratingRollout.migrate_out's layout
    assert starts.tolist() == [0, 5, 0, 5] and cap_out > 7 and n_send == 14
    starts, cap_out, n_send = mc.migrate_layout("short", cnt, 2)
    assert 0 < cap_out < 7 and 0 < n_send < 14
    assert mc.migrate_layout("shifted", cnt, 2)[0].tolist() == [-2, 3, -2, 3]


def test_references_by_definition_on_a_case_written_out():
    mask = mc.as_mask([0b101, 0b001, 0, 0b110, 0b101])
    at, live = mc.group_positions(mask, 3, [10, 20, 30])
    assert at.tolist() == [[10, -1, 30], [11, -1, -1], [-1, -1, -1], [-1, 20, 31], [12, -1, 32]]
    assert live.tolist() == (at >= 0).tolist()
    assert mc.block_counts(mask, 3).tolist() == [[3, 1, 3]] and mc.counts(mask, 3).tolist() == [3, 1, 3]
    assert mc.group_offsets_ref(np.array([[3, 1], [0, 2], [4, 0]]), [7, -1]).tolist() == [[7, -1], [10, 0], [10, 2]]
    recent = np.arange(20, dtype=np.float32).reshape(5, 4)
    out = mc.halo_pack_ref(recent, mask, [0, 3, 4], 6, mc.canary((6, 4)))
    assert out[:, 0].tolist() == [0.0, 4.0, 16.0, 12.0, 0.0, 12.0]             # the last place of group 2 (6) is refused
    hist = np.arange(2 * 6 * 4, dtype=np.float32).reshape(2, 6, 4)
    ids = np.arange(100, 106, dtype=np.int32)
    dest = np.array([1, 0, 5, 1, -1, 0], dtype=np.int32)
    h, i, s = mc.migrate_pack_ref(hist, 6, ids, dest, 2, 1, [0, 0], mc.canary((2, 1, 4)), mc.canary((1,), 7, np.int32),
                                  mc.canary((3, 3, 4)))
    assert i.tolist() == [100] and h[:, 0, 0].tolist() == [0.0, 24.0]         # row 3 is a stayer too: place 1 >= cap_out
    assert s[:2, 0, 0].view(np.int32).tolist() == [101, 105] and s[:2, 0, 1:].tolist() == [[0.0] * 3] * 2
    assert s[:2, 1:, 0].tolist() == [[4.0, 28.0], [20.0, 44.0]] and mc.same_bits(s[2], mc.canary((3, 3, 4))[2])
    h2, i2 = mc.migrate_unpack_ref(s[:2], mc.canary((2, 4, 4)), mc.canary((4,), 7, np.int32), 2)
    assert i2.tolist() == [7, 8, 101, 105] and h2[:, 2:, 0].tolist() == [[4.0, 20.0], [28.0, 44.0]]
    assert mc.same_bits(h2[:, :2], mc.canary((2, 4, 4))[:, :2])


def test_the_gate_compares_bits():
    a = np.array([1.0, np.nan, 0.0], dtype=np.float32)
    assert mc.same_bits(a, a.copy()) and mc.same_bits(torch.from_numpy(a), a)
    assert not mc.same_bits(a, np.array([1.0, np.nan, -0.0], dtype=np.float32))
    other_nan = a.copy()
    other_nan.view(np.int32)[1] ^= 1
    assert not mc.same_bits(a, other_nan)
    with pytest.raises(AssertionError, match="first at"):
        mc.assert_bits(a, other_nan, "nan payload")


# ---- exact problems are exact ---------------------------------------------------------------------------------------------
def test_the_restated_remainder_has_torchs_bits():
    """A zero keeps the dividend's sign (-box gives -0), a tiny negative dividend rounds up onto box itself."""
    for box in (1.0, 2.0):
        a = np.array([-2 * box, -box, -0.25, 0.0, 0.25, box, box + 0.5, 3 * box, -2.0 ** -30], dtype=np.float32)
        want = torch.remainder(torch.from_numpy(a), box).numpy()
        mc.assert_bits(mc._remainder(a, box, np.float32), want, "remainder")
        assert np.signbit(want[:2]).all() and not np.signbit(want[3]) and want[-1] == box
        mc.assert_bits(mc._remainder(a[:-1], box, np.float64).astype(np.float32), want[:-1], "remainder in float64")


def test_feature_problems_are_exact_in_float32():
    for w in mc.FEATURE_WINDOWS:
        for box in (1.0, 2.0):
            p = mc.features_problem(w, w, 257, w // 2, box)
            rows = np.arange(p["n_held"])
            x32, last32, _ = mc.features_eval(p["hist"], p["phase"], rows, p["n_held"], box, mc.DT, p["stats"], np.float32)
            x64, last64, _ = mc.features_eval(p["hist"], p["phase"], rows, p["n_held"], box, mc.DT, p["stats"], np.float64)
            assert np.array_equal(x32.astype(np.float64), x64) and np.array_equal(last32.astype(np.float64), last64)
            assert bool((last32 >= 0).all()) and bool((last32 < box).all()) and len(np.unique(x32)) > 20
            assert bool((p["hist"][:, :257, :3] < 0).any()) and bool((p["hist"][:, :257, :3] >= box).any())    # remainder works
            assert bool(np.isnan(p["hist"][:, 257:]).all())


def test_advance_problems_are_exact_in_float32_and_plant_every_face():
    for world, grid in mc.GRIDS.items():
        for use_planes in (False, True):
            for box in (1.0, 2.0):
                p = mc.advance_problem(world, 1025, 3, 1, grid, box, use_planes, permuted=True)
                args = (p["hist"], p["n"], p["phase"], p["pred_row"], p["acc"], p["rate"], mc.ADVANCE_STATS, mc.DT, box)
                new32 = mc.advance_eval(*args, np.float32)
                assert mc.same_bits(new32, p["want_new"])                      # one rounding per operation: the float64 answer
                assert mc.same_bits(mc.advance_eval(*args, np.float32, reciprocal=True), new32)
                lands = p["lands_on_box"]
                assert new32[lands, :3].tolist() == [box] * 3 and p["want_dest"][lands] == world - 1
                assert p["want_dest"][0] == 0 and p["want_new"][0, :3].tolist() == [0.0] * 3
                assert 0 <= p["want_dest"].min() and p["want_dest"].max() == world - 1
                # the planted rows stand still, and the two neighbours of a face or plane lie in different tiles
                targets = mc.planted_positions(grid, box, p["planes"])
                assert mc.same_bits(p["want_new"][p["planted"][:-1], :3], targets)
                tiles = mc.tile_of_ref(targets, grid, box, p["planes"])[1:].reshape(-1, 3)
                assert bool((tiles[:, 0] != tiles[:, 1]).all()) and bool((tiles[:, 1] == tiles[:, 2]).all())      # c_j <= v
                assert len(tiles) >= sum(g - 1 for g in grid)
    p = mc.advance_problem(3, 1, 3, 0, (2, 2, 2), 1.0, False, False)
    assert p["lands_on_box"] is None and p["want_dest"].tolist() == [0]


def test_tile_of_ref_restates_owner_of_on_odd_grids():
    """The float32 restatement against dist.owner_of's torch expression itself, on random and on planted positions."""
    gen = np.random.default_rng(5)
    for grid in ((3, 3, 3), (7, 3, 3), (1, 1, 5), (3, 2, 1), (4, 4, 4)):
        for box in (1.0, 2.0):
            v = np.concatenate([gen.random((4000, 3), dtype=np.float32) * np.float32(box), mc.planted_positions(grid, box, None),
                                np.full((1, 3), box, dtype=np.float32)])
            g = torch.tensor(grid, dtype=torch.float32)
            cell = torch.floor(torch.from_numpy(v) * np.float32(1.0 / box) * g).to(torch.int64)
            cell = torch.minimum(cell.clamp_min_(0), (g - 1).to(torch.int64))
            want = ((cell[:, 0] * grid[1] + cell[:, 1]) * grid[2] + cell[:, 2]).to(torch.int32).numpy()
            assert np.array_equal(mc.tile_of_ref(v, grid, box), want)


def test_halo_problems_are_exact_in_float32_and_plant_the_edge_of_reach():
    wrapped = 0
    for world in mc.WORLDS:
        for rank in {0, world - 1}:
            for margin in mc.HALO_MARGINS:
                for box in (1.0, 2.0):
                    p = mc.halo_problem(world + rank, 1025, world, rank, box, margin)
                    got32 = mc.peer_mask_eval(p["pos"], p["lo"], p["hi"], rank, p["margin"], box, np.float32)
                    assert np.array_equal(got32, p["want_mask"])
                    mask = [int(v) for v in p["want_mask"]]
                    assert all(m >> world == 0 and not (m >> rank) & 1 for m in mask)
                    if margin == "covers":                       # every axis skipped: every peer's bit on every row
                        assert set(mask) == {((1 << world) - 1) & ~(1 << rank)}
                    elif world > 1:
                        assert p["planted"] > 0 and len(set(mask)) > 1
                    wrapped += p["wrapped"]
    assert wrapped > 0
    # kept at exactly reach, dropped one STEP beyond: peer 0 of a 2 x 1 x 1 grid, seen from rank 1
    p = mc.halo_problem(1, 65, 2, 1, 1.0, "sixteenth")
    lo, hi = mc.dyadic_tiles((2, 1, 1), 1.0)
    assert lo[0].tolist() == [0, 0, 0] and hi[0].tolist() == [0.5, 1, 1]
    xs = p["pos"][mc._spread(65, 4), 0].astype(np.float64).tolist()
    step = 2.0 ** -mc.STEP_BITS
    assert xs == [1 - 0.0625, 1 - 0.0625 - step, 0.5625, 0.5625 + step]
    assert [int(v) for v in p["want_mask"][mc._spread(65, 4)]] == [1, 0, 1, 0]


# ---- ops.group_offsets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", (1, 64))
def test_group_offsets_is_the_definitional_prefix(world):
    gen = np.random.default_rng(world)
    for nb in (1, 2, 5):
        bc = gen.integers(0, 257, size=(nb, world)).astype(np.int32)
        bc[:, world // 2] = 0                                    # a group nobody belongs to
        starts = np.cumsum(bc.sum(axis=0)) - bc.sum(axis=0) - 3
        got = ops.group_offsets(torch.from_numpy(bc), torch.from_numpy(starts))
        assert got.dtype == torch.int32 and got.is_contiguous() and got.shape == (nb, world)
        assert np.array_equal(got.numpy(), mc.group_offsets_ref(bc, starts))
        assert got[:, world // 2].tolist() == [int(starts[world // 2])] * nb
    for n in mc.N_EDGES:                                         # on a mask's own counts, against the row's place itself
        mask = mc.mask_pattern("scattered", n, world)
        starts = mc.halo_layout("packed", mc.counts(mask, world))[0]
        off = ops.group_offsets(torch.from_numpy(mc.block_counts(mask, world)), torch.from_numpy(starts)).numpy()
        at, live = mc.group_positions(mask, world, starts)
        for b in range(mc.blocks(n)):
            rows = slice(b * mc.BLOCK, (b + 1) * mc.BLOCK)
            for p in range(world):
                first = at[rows, p][live[rows, p]]
                assert first.size == 0 or first[0] == off[b, p]


# ---- the gate tested on itself ------------------------------------------------------------------------------------------------
def _halo_pack_standin(c, defect=None):
    return mc.standin_halo_pack(c["rows"], c["mask"], c["world"], c["offsets"], c["n_out"], c["out0"][:c["n_out"]], defect)


def _migrate_standin(c, defect=None):
    return mc.standin_migrate_pack(c["hist"], c["n"], c["ids"], c["dest"], c["world"], c["rank"], c["offsets"], c["hist_out0"],
                                   c["ids_out0"], c["send0"][:c["n_send"]], defect)


def _migrate_equal(c, got):
    return mc.same_bits(got[0], c["want_hist_out"]) and mc.same_bits(got[1], c["want_ids_out"]) and \
        mc.same_bits(got[2], c["want_send"][:c["n_send"]])


@pytest.mark.parametrize("world", CPU_WORLDS)
def test_clean_counting_standin_equals_the_definition(world):
    for name in mc.MASK_PATTERNS:
        for n in mc.N_EDGES:
            mask = mc.mask_pattern(name, n, world)
            bc, cnt = mc.standin_counts(mask, world)
            assert np.array_equal(bc, mc.block_counts(mask, world)) and np.array_equal(cnt, mc.counts(mask, world)), (name, n)
            by_rows = [sum((int(m) >> p) & 1 for m in mask) for p in range(world)]
            assert cnt.tolist() == by_rows
    for name in mc.DEST_PATTERNS:                                # cgnn_rollout_advance counts one bit per row
        for n in mc.N_EDGES:
            dest = mc.dest_pattern(name, n, world, world - 1)
            bc, cnt = mc.standin_counts(mc.dest_mask(dest, world), world)
            assert cnt.tolist() == [int((dest == p).sum()) for p in range(world)] and bc.sum(axis=0).tolist() == cnt.tolist()


@pytest.mark.parametrize("world", CPU_WORLDS)
def test_clean_halo_pack_standin_equals_the_definition(world):
    for name in mc.MASK_PATTERNS:
        for n in mc.N_EDGES:
            for layout in mc.START_LAYOUTS:
                c = mc.halo_pack_case(name, n, world, layout)
                assert mc.same_bits(_halo_pack_standin(c), c["want"][:c["n_out"]]), (name, n, layout)


@pytest.mark.parametrize("world", (1, 2, 64))
def test_clean_migrate_pack_standin_equals_the_definition(world):
    for name in mc.DEST_PATTERNS:
        for n in mc.N_EDGES:
            for rank in sorted({0, world - 1}):
                for layout in mc.START_LAYOUTS:
                    c = mc.migrate_pack_case(name, n, world, rank, 2 + 3 * (n % 2), layout)
                    assert _migrate_equal(c, _migrate_standin(c)), (name, n, rank, layout)


def test_every_planted_defect_is_caught_by_a_named_pattern(capsys):
    """The gate on itself: per defect, the patterns whose comparison fails (sizes 257 and 513, world 64)."""
    caught = {d: set() for d in mc.DEFECTS}
    world = 64
    for defect in mc.DEFECTS:
        for n in (257, 513):
            for name in mc.MASK_PATTERNS:
                mask = mc.mask_pattern(name, n, world)
                bc, cnt = mc.standin_counts(mask, world, defect)
                if not (np.array_equal(bc, mc.block_counts(mask, world)) and np.array_equal(cnt, mc.counts(mask, world))):
                    caught[defect].add(f"counts:{name}")
                for layout in mc.START_LAYOUTS:
                    c = mc.halo_pack_case(name, n, world, layout)
                    if not mc.same_bits(_halo_pack_standin(c, defect), c["want"][:c["n_out"]]):
                        caught[defect].add(f"halo_pack:{name}:{layout}")
            for name in mc.DEST_PATTERNS:
                for layout in mc.START_LAYOUTS:
                    c = mc.migrate_pack_case(name, n, world, world - 1, 5, layout)
                    if not _migrate_equal(c, _migrate_standin(c, defect)):
                        caught[defect].add(f"migrate_pack:{name}:{layout}")
    with capsys.disabled():
        for defect, names in caught.items():
            print(f"\n  {defect}: caught by {len(names)} cases, e.g. {sorted(names)[:4]}", end="")
    for defect, names in caught.items():
        assert names, f"no pattern catches {defect}"
    kernels = lambda d: {n.split(":")[0] for n in caught[d]}                  # noqa: E731
    assert kernels("rank_counts_le") == kernels("wave_sum_through_own_wave") == {"halo_pack", "migrate_pack"}
    assert kernels("offsets_of_next_workgroup") == {"halo_pack", "migrate_pack"}
    assert kernels("bit_63_dropped") == {"counts", "halo_pack", "migrate_pack"}
    assert "halo_pack:top_bit:packed" in caught["bit_63_dropped"]
    assert kernels("send_slots_rotated") == {"migrate_pack"}
    assert caught["refused_row_takes_no_place"] and all(n.endswith(":shifted") for n in caught["refused_row_takes_no_place"])
