"""CPU, every run: the decomposition kernels' geometry restated in tests/decompose_checks.py pinned against csrc/decompose.hip,
csrc/cgnn_common.hpp and (where the library loads) ``cgnn_balanced_planes_workspace_bytes``; every value family shown to be what
its name says, by its key bits; the arbitrary-grid references held to ``dist.balanced_planes`` / ``owner_of`` / ``_near_tile``
and to the brute force of tests/test_balanced_decomposition_cpu.py; the planted mask problems shown to be exact; and the gate
tested on itself: stand-ins that follow the kernels' chunks, digit passes, trips and LDS count tables equal the references on
every family at every size of ``N_EDGES`` on every grid (the block cap lowered to 1, so that two trips happen above 1024
rows), and every planted defect is caught by at least one named case."""
import os
import re

import numpy as np
import pytest
import torch

import decompose_checks as dc
from cosmology_gnn_simulation_amd import _lib, dist as cdist
from test_balanced_decomposition_cpu import brute_force_owner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(text, name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1))


# ---- pinned numbers ----------------------------------------------------------------------------------------------------
def test_geometry_is_the_kernels_and_the_librarys():
    kernel = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "decompose.hip")).read()
    common = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "cgnn_common.hpp")).read()
    assert dc.BINS == _define(kernel, "CGNN_DEC_BINS") == 1 << dc.DIGITS[0][1]
    assert dc.CHUNK == _define(kernel, "CGNN_DEC_CHUNK") and dc.MAX_WORLD == _define(kernel, "CGNN_DEC_MAX_WORLD")
    assert dc.MAX_BLOCKS == _define(kernel, "CGNN_DEC_MAX_BLOCKS") and dc.BATCH == _define(kernel, "CGNN_DEC_BATCH")
    assert dc.BLOCK == _define(common, "CGNN_BLOCK")
    assert re.search(r"shift_of\[3\] = \{21, 10, 0\}, bits_of\[3\] = \{11, 11, 10\}", kernel)
    assert dc.DIGITS == ((21, 11), (10, 11), (0, 10)) and sum(b for _, b in dc.DIGITS) == 32
    assert all(s == sum(b for _, b in dc.DIGITS[i + 1:]) for i, (s, _) in enumerate(dc.DIGITS))
    assert "(n + 4 * CGNN_BLOCK - 1) / (4 * CGNN_BLOCK)" in kernel
    assert [dc.blocks(n) for n in (0, 1, 1024, 1025, 2048 * 1024, 2048 * 1024 + 1, 10 ** 7)] == [1, 1, 1, 2, 2048, 2048, 2048]
    assert dc.FIRST_N_WITH_TWO_TRIPS == 2_097_153
    assert dc.trips(dc.FIRST_N_WITH_TWO_TRIPS - 1) == 1 and dc.trips(dc.FIRST_N_WITH_TWO_TRIPS) == 2
    assert dc.trips(dc.N_TWO_TRIPS) == 2 and dc.N_TWO_TRIPS == 2_097_152 + 1025 + 3
    assert [dc.trips(n, 1) for n in dc.N_EDGES] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 5]
    assert dc.N_EDGES == (1, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
    # the workspace: struct DecTarget { uint32_t; int32_t }, every region aligned to 256 bytes
    assert re.search(r"struct DecTarget \{\s*uint32_t prefix;[^}]*int32_t rank;[^}]*\};", kernel) and dc.TARGET_BYTES == 8
    lay = dc.dec_layout(100, 8)
    assert (lay["part"], lay["count"], lay["target"], lay["hist"], lay["total"]) == (0, 512, 768, 1024, 1024 + 7 * 2048 * 4)
    assert dc.dec_layout(0, 1)["total"] == 256 + 256 + 256 + 2048 * 4 and dc.dec_layout(5, 1)["max_targets"] == 1
    try:
        lib = _lib.load()
    except Exception:                                            # no library without a GPU runtime: the restated layout alone
        lib = None
    if lib is not None:
        for grid in dc.GRIDS:
            for n in (0, 1, 63, 64, 65, 4097, dc.N_TWO_TRIPS):
                assert lib.cgnn_balanced_planes_workspace_bytes(n, *grid) == dc.dec_layout(n, dc.world_of(grid))["total"]
        assert lib.cgnn_balanced_planes_workspace_bytes(10, 4097, 1, 1) == 0


def test_the_grids_reach_every_chunk_shape():
    need = {(1, 1, 1), (2, 1, 1), (1, 3, 1), (1, 1, 5), (2, 1, 2), (3, 2, 1), (5, 1, 1), (6, 1, 1), (2, 5, 1), (4, 4, 4), (3, 3, 3),
            (7, 3, 3), (4, 2, 2), (16, 16, 16), (4096, 1, 1)}
    assert need <= set(dc.GRIDS) and set(dc.TWO_TRIP_GRIDS) == {(2, 2, 2), (4, 4, 4)} <= set(dc.GRIDS)
    assert max(dc.world_of(g) for g in dc.GRIDS) == dc.MAX_WORLD

    def levels(grid):                                           # (segments, targets per segment) of every split level
        seg, out = 1, []
        for p in grid:
            if p > 1:
                out.append((seg, p - 1))
            seg *= p
        return out
    assert levels((5, 1, 1)) == [(1, dc.CHUNK)] and levels((6, 1, 1)) == [(1, dc.CHUNK + 1)]
    assert levels((2, 5, 1))[1] == (2, dc.CHUNK)                 # aligned: segment s owns chunk s
    seg, per = levels((4, 4, 4))[1]
    straddling = [s for s in range(seg) if (s * per) // dc.CHUNK != (s * per + per - 1) // dc.CHUNK]
    assert per == 3 and straddling == [1, 2]                     # segment 1 owns targets 3..5
    assert any(seg * per > dc.CHUNK and seg * per % dc.CHUNK for g in dc.GRIDS for seg, per in levels(g))    # nt < 4
    # a count table beyond 256 entries that the next level reads (assign), and the largest (classify)
    assert [s for s, _ in levels((17, 16, 2))][2] == 272 > dc.BLOCK and dc.world_of((16, 16, 16)) == dc.MAX_WORLD


# ---- the key map and the families ------------------------------------------------------------------------------------------
def test_the_key_map_orders_floats_and_folds_minus_zero():
    v = np.array([-np.inf, -dc.FLT_MAX, -1.0, -dc.DENORM, -0.0, 0.0, dc.DENORM, 1.0, dc.FLT_MAX, np.inf], dtype=np.float32)
    k = dc.dec_key(v)
    assert k[4] == k[5] == 0x80000000 and bool((np.diff(k.astype(np.int64))[[0, 1, 2, 3, 5, 6, 7, 8]] > 0).all())
    back = dc.dec_unkey(k)
    assert dc.same_bits(back, np.where(v == 0, np.float32(0.0), v).astype(np.float32))
    gen = np.random.default_rng(0)
    r = gen.integers(0, 2 ** 32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[~np.isnan(r)]
    order = np.argsort(dc.dec_key(r), kind="stable")
    assert np.array_equal(r[order] + np.float32(0), np.sort(r) + np.float32(0))
    assert dc.same_bits(dc.dec_unkey(dc.dec_key(r)), np.where(r == 0, np.float32(0.0), r).astype(np.float32))
    assert dc.digits_of(np.array([0xFFFFFFFF], dtype=np.uint32)) == (2047, 2047, 1023)


def test_value_families_are_what_their_names_say():
    nb = len(dc.FINITE_TOP_BINS)
    assert nb == 2040
    for n in dc.N_EDGES:
        for seed in range(3):
            fam = {name: dc.family(name, n, 4, seed) for name in dc.FAMILIES if name != "clustered"}
            assert all(v.dtype == np.float32 and v.shape == (n,) and not np.isnan(v).any() for v in fam.values())
            top, mid, low = dc.digits_of(dc.dec_key(fam["low_digit"]))
            assert len(set(top)) == 1 and len(set(mid)) == 1 and (n < 255 or len(set(low)) > 100)
            top, mid, low = dc.digits_of(dc.dec_key(fam["mid_digit"]))
            assert len(set(top)) == 1 and set(low) == {0} and (n < 255 or len(set(mid)) > 100)
            v = fam["one_per_top_bin"]
            top, _, _ = dc.digits_of(dc.dec_key(v))
            assert len(np.unique(v)) == n and set(top) <= set(dc.FINITE_TOP_BINS) and bool(np.isfinite(v).all())
            assert bool((v != 0).all()) and (n < 255 or (bool((v < 0).any()) and bool((v > 0).any())))
            if n <= nb:                                          # a bin count of 1: every rank sits at before == rank
                assert len(set(top)) == n
            else:
                assert len(set(top)) == nb and np.bincount(top).max() == -(-n // nb)
            top, mid, low = dc.digits_of(dc.dec_key(fam["digit_edges"]))
            assert set(mid) <= {0, 2047} and set(low) <= {0, 1023} and bool(np.isfinite(fam["digit_edges"]).all())
            assert n < 255 or (set(mid) == {0, 2047} and set(low) == {0, 1023} and len(set(top)) == 8)
            assert len(set(fam["all_equal"])) == 1
            assert len(set(fam["two_values"])) == (2 if n >= 255 else len(set(fam["two_values"]))) <= 2
            z = fam["signed_zeros"]
            assert bool((np.abs(z) <= 2 * dc.DENORM).all())
            assert n < 255 or (len(set(z.view(np.int32))) == 6 and bool(np.signbit(z[z == 0]).any())
                               and not bool(np.signbit(z[z == 0]).all()))
            e = fam["extremes"]
            assert n < 255 or ({-np.inf, np.inf, float(dc.FLT_MAX), -float(dc.FLT_MAX), float(dc.DENORM), 2.5, -1.25}
                               <= set(e.tolist()) and bool(np.signbit(e[e == 0]).any()))
    assert dc.same_bits(dc.family("two_values", 300, 2, 2).max(), np.nextafter(np.float32(0.5), np.float32(1)))
    pos = dc.frame("clustered", 257, (2, 2, 2))
    assert pos.shape == (257, 3) and pos.min() >= 0 and pos.max() < 1
    for name in dc.FAMILIES:
        pos = dc.frame(name, 1025, (4, 4, 4), seed=3)
        assert pos.dtype == np.float32 and pos.shape == (1025, 3) and pos.flags["C_CONTIGUOUS"] and not np.isnan(pos).any()
        if name not in ("clustered", "ties_across_rank"):
            assert np.array_equal(np.sort(pos[:, 0]), np.sort(pos[:, 2]))
            assert name == "all_equal" or not np.array_equal(pos[:, 0], pos[:, 2])


def test_ties_across_rank_hit_the_first_an_interior_and_the_last_element_of_a_run():
    for n in (255, 257, 1025, 4097):
        for p in (2, 3, 4, 5, 7, 16):
            for shift in range(3):
                s = np.sort(dc.family("ties_across_rank", n, p, shift))
                assert np.array_equal(np.unique(s, return_inverse=True)[1], dc.tie_runs(n, p, shift) - 0)
                kinds = set()
                for j in range(1, p):
                    r = (j * n) // p
                    run = np.nonzero(s == s[r])[0]
                    kind = dc.TIE_KINDS[(j + shift) % 3]
                    assert len(run) >= 2 and {"first": r == run[0], "last": r == run[-1],
                                              "interior": run[0] < r < run[-1]}[kind], (n, p, j, kind, run, r)
                    kinds.add(kind)
                assert len(kinds) == min(3, p - 1)


# ---- the references ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", (1, 2, 3, 4, 6, 8, 12, 27))
def test_the_arbitrary_grid_reference_equals_the_torch_restatement_and_the_brute_force(world):
    grid = cdist.tile_grid(world)
    for name in dc.FAMILIES:
        for n in (3, 257, 2049):
            pos = dc.frame(name, n, grid, seed=world)
            t = torch.from_numpy(pos)
            want = cdist.balanced_planes(t, 1.0, world)
            cx, cy, cz, owner = dc.planes_ref(pos, grid)
            for g, w in zip((cx, cy, cz), want.tensors()):
                dc.assert_bits(g, w, f"planes {name} world {world} n {n}")
            want_owner = cdist.owner_of(t, 1.0, world, want)
            dc.assert_bits(owner, want_owner, f"owner {name} world {world} n {n}")
            dc.assert_bits(dc.owner_ref(pos, (cx, cy, cz)), want_owner, "owner_ref")
            assert np.array_equal(owner.astype(np.int64), brute_force_owner(t, world))
            assert dc.counts_ref(owner, world).tolist() == torch.bincount(want_owner.long(), minlength=world).tolist()
            for rank in dc.mask_ranks(world):
                lo, hi = dc.bounds_ref((cx, cy, cz), grid, rank, 1.0)
                assert (lo, hi) == cdist.tile_bounds(1.0, world, rank, want)
                for margin in (0.004, 0.07, 0.6):
                    near = cdist._near_tile(t, 1.0, lo, hi, margin)
                    got = dc.near_tile_eval(pos, lo, hi, margin, 1.0, np.float32)
                    assert np.array_equal(got, near.numpy()), (name, world, n, rank, margin)
                    assert np.array_equal(dc.mask_ref(pos, owner, rank, lo, hi, margin, 1.0),
                                          (near | (want_owner == rank)).numpy().astype(np.uint8))


def test_the_reference_on_a_case_written_out():
    pos = np.array([[0.5, 3, 0], [0.25, 1, 0], [-0.0, 2, 0], [0.75, 0, 0], [0.0, 5, 0], [0.25, 4, 0]], dtype=np.float32)
    cx, cy, cz, owner = dc.planes_ref(pos, (3, 2, 1))            # sorted x: -0 0 .25 .25 .5 .75 -> s[2], s[4]
    assert cx.tolist() == [0.25, 0.5] and owner.tolist() == [5, 2, 0, 4, 1, 3]
    assert cy.tolist() == [[5.0], [4.0], [3.0]] and cz.shape == (3, 2, 0)          # slabs {2, 5}, {1, 4}, {3, 0}
    cx, _, _, owner = dc.planes_ref(np.zeros((2, 3), dtype=np.float32) * np.float32(-1), (2, 2, 1))
    assert dc.same_bits(cx, np.zeros(1, dtype=np.float32)) and owner.tolist() == [3, 3]
    _, cy, _, _ = dc.planes_ref(np.full((2, 3), 7, dtype=np.float32), (2, 2, 1))
    assert cy.tolist() == [[0.0], [7.0]]                          # the empty slab: zeros are stored
    long_row = dc.hand_planes((4096, 1, 1), 2.0)[0]              # bisection over one long ascending row counts like the loop
    v = np.concatenate([dc.frame("extremes", 4097, (2, 1, 1))[:, 0], long_row[::7], np.nextafter(long_row[::5], np.float32(9))])
    assert np.array_equal(dc.part_of(long_row, v), dc.part_of(long_row, v, loop=True)) and dc.part_of(long_row, v).max() == 4095
    for n in (1, 2, 255, 1024, 4097, 1_000_003):
        assert np.array_equal(np.sort(dc._shuffle(n, n % 5)), np.arange(n))
    assert dc.bounds_ref((np.array([0.25, 0.5]), np.array([[5.0], [4.0], [3.0]]), np.zeros((3, 2, 0))), (3, 2, 1), 3, 8.0) == \
        ([0.25, 4.0, 0.0], [0.5, 8.0, 8.0])


# ---- mask problems -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", dc.GRIDS, ids=dc.grid_id)
def test_mask_problems_are_exact_and_plant_every_edge(grid):
    world = dc.world_of(grid)
    split = [a for a in range(3) if grid[a] > 1]
    for box in (1.0, 2.0):
        planes = dc.hand_planes(grid, box)
        for c in planes:
            assert dc.same_bits(c.astype(np.float64) * (1 << dc.PLANE_BITS) / box % 1, np.zeros(c.shape))
        if max(grid) >= 3:                                       # duplicate planes: parts nobody can lie in
            assert any(bool((np.diff(c.reshape(-1, c.shape[-1]), axis=1) == 0).any()) for c in planes if c.shape[-1] > 1)
        for rank in dc.mask_ranks(world):
            for name in dc.MARGINS:
                p = dc.mask_problem(world + rank, 1025, grid, box, rank, name)
                lo, hi, margin = p["lo"], p["hi"], p["margin"]
                tested = [a for a in range(3) if (hi[a] - lo[a]) + 2 * margin < box]
                if name == "covers" or (name == "closes" and len(split) <= 1):
                    assert tested == [] and bool(p["want_mask"].all())
                if name == "closes" and split:
                    assert (hi[split[0]] - lo[split[0]]) + 2 * margin == box and split[0] not in tested
                if name == "closes_less" and split:
                    a = split[0]
                    assert a in tested and np.float32(0.5 * (hi[a] - lo[a]) + margin) == np.float32(box / 2 - box * 2.0 ** -20)
                # exact: the float64 evaluation gives the float32 bits on the exact rows and on the lattice rows
                near32 = dc.near_tile_eval(p["pos"], lo, hi, margin, box, np.float32)
                near64 = dc.near_tile_eval(p["pos"], lo, hi, margin, box, np.float64)
                exact = np.ones(p["n"], dtype=bool)
                exact[np.arange(p["planted"]) * (p["n"] // p["planted"])] = False
                exact[p["exact_rows"]] = True
                assert np.array_equal(near32[exact], near64[exact])
                # at a reach: kept; one step towards the centre: kept; one step beyond: dropped
                rows = p["exact_rows"]
                assert len(rows) == 6 * len(tested)
                if len(tested) == 1:                             # (a tile between duplicate planes has no width: no inside)
                    kept = near32[rows].reshape(2, 3).tolist()
                    a = tested[0]
                    inside = [True] if 0.5 * (hi[a] - lo[a]) + margin > 0 else [False]
                    assert kept == [[False, True] + inside, inside + [True, False]], (grid, rank, name, kept)
                assert p["want_counts"].sum() == 1025 and p["want_counts"].dtype == np.int64
        # the two float32 neighbours of a plane value lie in different parts, the value itself in the upper one
        rows = dc.plane_rows(planes, grid, box)
        tiles = dc.owner_ref(rows, planes)[1:].reshape(-1, 3)
        assert bool((tiles[:, 0] != tiles[:, 1]).all()) and bool((tiles[:, 1] == tiles[:, 2]).all())
        assert len(tiles) >= sum(min(g - 1, 1) for g in grid) and dc.owner_ref(rows, planes)[0] == 0


# ---- the gate tested on itself -------------------------------------------------------------------------------------------------
def _planes_equal(got, want):
    return all(dc.same_bits(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("grid", dc.GRIDS, ids=dc.grid_id)
def test_clean_standins_equal_the_references(grid):
    """Every family at every size of N_EDGES, one block of 256 threads: two trips from 1025 rows on, five at 4097."""
    world = dc.world_of(grid)
    for name in dc.FAMILIES:
        for n in dc.N_EDGES:
            pos = dc.frame(name, n, grid, seed=n % 3)
            want = dc.planes_ref(pos, grid)
            got = dc.standin_planes(pos, grid, max_blocks=1)
            assert _planes_equal(got, want), (name, n)
            if n in (3, 257, 1025):                              # owner == NULL: the last level is not assigned
                assert _planes_equal(dc.standin_planes(pos, grid, want_owner=False, max_blocks=1)[:3], want[:3]), (name, n)
            rank = world // 2
            lo, hi = dc.bounds_ref(want[:3], grid, rank, 1.0)
            owner, counts, mask = dc.standin_classify(pos, want[:3], rank, lo, hi, 0.07, 1.0, max_blocks=1)
            assert dc.same_bits(owner, want[3]) and dc.same_bits(counts, dc.counts_ref(want[3], world))
            assert dc.same_bits(mask, dc.mask_ref(pos, want[3], rank, lo, hi, 0.07, 1.0))
    assert _planes_equal(dc.standin_planes(dc.frame("clustered", 4097, grid), grid), dc.planes_ref(dc.frame("clustered", 4097, grid), grid))


# the named cases: (family, n, grid, block cap); every defect must be caught by the cases listed for it, and by no case
# listed under "blind"
CASES = {
    "full_chunk": ("clustered", 1025, (5, 1, 1), dc.MAX_BLOCKS),
    "chunk_of_one": ("clustered", 1025, (6, 1, 1), dc.MAX_BLOCKS),
    "aligned": ("clustered", 1025, (2, 5, 1), dc.MAX_BLOCKS),
    "straddling": ("clustered", 1025, (4, 4, 4), dc.MAX_BLOCKS),
    "signed_zeros": ("signed_zeros", 257, (3, 2, 1), dc.MAX_BLOCKS),
    "extremes": ("extremes", 1025, (4, 2, 2), dc.MAX_BLOCKS),
    "top_bins": ("one_per_top_bin", 1023, (7, 3, 3), dc.MAX_BLOCKS),
    "two_trips": ("clustered", 1025, (2, 2, 2), 1),
    "one_trip": ("clustered", 1024, (2, 2, 2), 1),
    "empty_slabs": ("all_equal", 257, (3, 3, 3), dc.MAX_BLOCKS),
    "fewer_than_tiles": ("clustered", 3, (2, 2, 2), dc.MAX_BLOCKS),
    "ties": ("ties_across_rank", 1025, (7, 3, 3), dc.MAX_BLOCKS),
    "one_level": ("clustered", 257, (1, 3, 1), dc.MAX_BLOCKS),
    "wide_assign": ("clustered", 4097, (17, 16, 2), dc.MAX_BLOCKS),
    "max_cube": ("clustered", 4097, (16, 16, 16), dc.MAX_BLOCKS),
    "max_slabs": ("clustered", 4097, (4096, 1, 1), dc.MAX_BLOCKS),
}
CATCHES = {                                                      # defect: (planes cases that must catch, planes cases that cannot)
    "flush_drops_t0": ({"chunk_of_one", "aligned", "straddling", "max_cube"}, {"full_chunk", "one_level"}),
    "overlap_off_by_one": ({"chunk_of_one", "straddling"}, {"full_chunk", "aligned"}),
    "rank_not_reduced": ({"straddling", "top_bins", "ties"}, set()),
    "last_digit_11_bits": ({"full_chunk", "straddling", "extremes"}, set()),
    "minus_zero_not_folded": ({"signed_zeros"}, {"straddling", "two_trips"}),
    "negative_keys_not_inverted": ({"extremes", "top_bins"}, {"straddling", "aligned"}),
    "second_trip_dropped": ({"two_trips"}, {"one_trip", "straddling"}),
    "empty_rank_is_zero": ({"empty_slabs", "fewer_than_tiles"}, {"straddling", "full_chunk"}),
    "part_counts_lt": ({"straddling", "ties", "one_level"}, set()),
    "stale_count_buffer": ({"straddling", "aligned", "two_trips"}, {"one_level", "full_chunk"}),
    "lds_flush_one_trip": ({"wide_assign"}, {"straddling", "max_cube", "max_slabs"}),
}
CLASSIFY_CATCHES = {"second_trip_dropped": {"two_trips"}, "part_counts_lt": {"straddling", "ties"},
                    "lds_flush_one_trip": {"wide_assign", "max_cube", "max_slabs"}}


def test_every_planted_defect_is_caught_by_a_named_case(capsys):
    """The gate on itself: per defect, the named cases whose comparison fails.  The last level's counts of
    cgnn_balanced_planes are read by nobody, so a lost LDS flush shows there only on a grid whose middle level has more
    than 256 segments (17 x 16 x 2); cgnn_tile_classify's counts show it on every grid above 256 tiles."""
    assert set(CATCHES) == set(dc.DEFECTS) and len(dc.DEFECTS) == 11
    caught = {d: set() for d in dc.DEFECTS}
    caught_classify = {d: set() for d in dc.DEFECTS}
    for case, (name, n, grid, cap) in CASES.items():
        pos = dc.frame(name, n, grid)
        want = dc.planes_ref(pos, grid)
        world = dc.world_of(grid)
        assert _planes_equal(dc.standin_planes(pos, grid, max_blocks=cap), want), case
        lo, hi = dc.bounds_ref(want[:3], grid, world - 1, 1.0)
        want_c = (want[3], dc.counts_ref(want[3], world), dc.mask_ref(pos, want[3], world - 1, lo, hi, 0.07, 1.0))
        for defect in dc.DEFECTS:
            if not _planes_equal(dc.standin_planes(pos, grid, defect=defect, max_blocks=cap), want):
                caught[defect].add(case)
            got = dc.standin_classify(pos, want[:3], world - 1, lo, hi, 0.07, 1.0, defect=defect, max_blocks=cap)
            if not _planes_equal(got, want_c):
                caught_classify[defect].add(case)
    with capsys.disabled():
        for defect in dc.DEFECTS:
            print(f"\n  {defect}: planes {sorted(caught[defect])}; classify {sorted(caught_classify[defect])}", end="")
    for defect, (must, blind) in CATCHES.items():
        assert must <= caught[defect], (defect, must - caught[defect])
        assert not blind & caught[defect], (defect, blind & caught[defect])
    for defect in dc.DEFECTS:
        assert CLASSIFY_CATCHES.get(defect, set()) <= caught_classify[defect], defect
        if defect not in CLASSIFY_CATCHES:
            assert not caught_classify[defect], defect         # the classify stand-in has no such step
