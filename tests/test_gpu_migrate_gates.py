"""GPU: the six kernels of csrc/migrate.hip gated EXACTLY at every lane, wave, workgroup and world edge (tests/migrate_checks.py;
the gates are tested on themselves in tests/test_migrate_gates_cpu.py).  Every comparison is bit equality through an integer
view, NaN padding and canaries included; there are no tolerances.  The placement kernels run the named mask and destination
patterns at every size of ``N_EDGES`` against references written by definition (a group's rows, ascending, get consecutive
places); the float kernels run problems on which every float32 operation is exact, so a float64 evaluation is the answer.
Outputs that must keep canaries are pre-filled here and handed to the C entries directly (the ``ops`` wrappers allocate with
``torch.empty``); inputs lie between NaN rows.

Sizes: no case has more than 1025 rows or 64 x 1025 output rows.  Left to tests/test_gpu_migrating_rollout.py: the parity of
cgnn_rollout_advance and cgnn_history_features with the torch expressions on random inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import migrate_checks as mc
from cosmology_gnn_simulation_amd import _lib, ops
from reduction_checks import PAD_ROWS

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = -1                    # CGNN_ERR_INVALID_ARG


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mask_t(mask):
    return _dev(np.ascontiguousarray(mask, dtype=np.uint64).view(np.int64))


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _inner(full):
    """The rows between the NaN rows of a ``mc.padded`` tensor on the device: the contiguous view the kernels get."""
    v = full[PAD_ROWS:full.shape[0] - PAD_ROWS]
    assert v.is_contiguous()
    return v


# ---- cgnn_halo_select ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", mc.WORLDS)
def test_halo_select_sets_exactly_the_peers_within_reach(world):
    """Dyadic tiles on GRIDS[world]; margins 0, 1/16 and one that covers every split axis (every peer's bit on every row: 63
    bits at world 64, bit 63 among them); points planted at exactly ``reach`` and one step beyond, through the periodic wrap
    too.  The mask, every row of block_counts and counts; the own bit and the bits >= world are never set."""
    lib = _lib.load()
    for rank in sorted({0, world - 1}):
        for margin in mc.HALO_MARGINS:
            for n, box in ((65, 2.0), (257, 1.0), (1025, 2.0)):
                p = mc.halo_problem(100 * world + rank, n, world, rank, box, margin)
                recent = _dev(mc.padded(p["recent"]))
                boxes = ops.tile_boxes(p["lo"].tolist(), p["hi"].tolist())
                mask, bc, cnt = ops.halo_select(_inner(recent), rank, boxes, p["margin"], box)
                got = mask.cpu().numpy().view(np.uint64)
                what = f"halo_select world {world} rank {rank} margin {margin} n {n}"
                mc.assert_bits(got, p["want_mask"], what)
                assert not bool(mc.has_bit(got, rank).any()), what
                assert world == 64 or not bool((got >> np.uint64(world)).any()), what
                mc.assert_bits(bc, mc.block_counts(p["want_mask"], world), what + " block_counts")
                mc.assert_bits(cnt, mc.counts(p["want_mask"], world), what + " counts")
                if margin == "covers" and world == 64 and rank == 0:
                    assert bool(mc.has_bit(got, 63).all()) and bool((mask < 0).all())        # the int64 tensor's sign bit
                # the same call through the entry, with canaries behind every output
                mask0 = mc.canary((n + PAD_ROWS,), 1 << 40, np.int64)
                bc0 = mc.canary((mc.blocks(n) + 1, world), 1 << 20, np.int32)
                cnt0 = mc.canary((world + 8,), 1 << 20, np.int32)
                mask_d, bc_d, cnt_d = _dev(mask0), _dev(bc0), _dev(cnt0)
                assert lib.cgnn_halo_select(_inner(recent).data_ptr(), n, world, rank, boxes[0], boxes[1], p["margin"], box,
                                            mask_d.data_ptr(), bc_d.data_ptr(), cnt_d.data_ptr(), _stream()) == 0
                mask0[:n] = p["want_mask"].view(np.int64)
                bc0[:-1] = mc.block_counts(p["want_mask"], world)
                cnt0[:world] = mc.counts(p["want_mask"], world)
                mc.assert_bits(mask_d, mask0, what + " mask and canaries")
                mc.assert_bits(bc_d, bc0, what + " block_counts and canaries")
                mc.assert_bits(cnt_d, cnt0, what + " counts and canaries")


# ---- cgnn_halo_pack --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", mc.HALO_PACK_WORLDS)
@pytest.mark.parametrize("name", mc.MASK_PATTERNS)
def test_halo_pack_places_every_row_of_every_group(name, world):
    """Every mask pattern at every size of N_EDGES: groups back to back, an n_out that cuts the tail off (``at < n_out``) and
    starts 3 lower (``at >= 0``: the skipped rows still count).  Rows beyond a group's end and beyond n_out keep their
    canary; ``recent`` lies between NaN rows."""
    lib = _lib.load()
    for n in mc.N_EDGES:
        for layout in mc.START_LAYOUTS:
            c = mc.halo_pack_case(name, n, world, layout)
            recent, mask, out = _dev(c["recent"]), _mask_t(c["mask"]), _dev(c["out0"])
            offsets = ops.group_offsets(_dev(mc.block_counts(c["mask"], world)), _dev(c["starts"]))
            mc.assert_bits(offsets, c["offsets"], "group_offsets")
            assert lib.cgnn_halo_pack(_inner(recent).data_ptr(), mask.data_ptr(), n, world, offsets.data_ptr(), c["n_out"],
                                      out.data_ptr(), _stream()) == 0
            mc.assert_bits(out, c["want"], f"halo_pack {name} world {world} n {n} {layout}")
    c = mc.halo_pack_case(name, 257, world, "packed")             # the wrapper: the same rows
    rows = ops.halo_pack(_dev(c["rows"]), _mask_t(c["mask"]), _dev(c["offsets"]), c["n_out"])
    mc.assert_bits(rows, c["want"][:c["n_out"]], f"ops.halo_pack {name} world {world}")


# ---- cgnn_rollout_advance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", ("uniform", "planes"))
@pytest.mark.parametrize("world", sorted(mc.GRIDS))
def test_rollout_advance_lands_every_row_in_its_tile(world, tiles):
    """Every grid of GRIDS, equal-volume tiles and planes, every phase of a W = 3 ring (s1 and s2 wrap), identity and permuted
    prediction rows.  Planted: the origin, every interior face / a plane value of the row's own column exactly (``c_j <= v``),
    its float32 neighbours on both sides, and a row whose wrapped position is box itself.  The record, the whole ring (the
    other slots and the rows >= n_held keep their bits), dest, every row of block_counts, counts; canaries behind each."""
    lib = _lib.load()
    grid = mc.GRIDS[world]
    stats = (C.c_float * 8)(*mc.ADVANCE_STATS)
    w = mc.ADVANCE_WINDOW
    for n in mc.ADVANCE_N:
        for phase in range(w):
            for permuted in (False, True):
                box = (1.0, 2.0)[(n + phase) % 2]
                p = mc.advance_problem(7 * n + phase, n, w, phase, grid, box, tiles == "planes", permuted)
                what = f"advance grid {grid} {tiles} n {n} phase {phase} permuted {permuted} box {box}"
                hist, ids = _dev(p["hist"]), _dev(p["ids"])
                acc, rate = _dev(mc.padded(p["acc"])), _dev(mc.padded(p["rate"]))
                pred_row = None if p["pred_row"] is None else _dev(p["pred_row"])
                planes = [None] * 3 if p["planes"] is None else [_dev(c) for c in p["planes"]]
                record0 = mc.canary((n + PAD_ROWS, mc.ROW))
                dest0 = mc.canary((n + PAD_ROWS,), 1 << 20, np.int32)
                bc0 = mc.canary((mc.blocks(n) + 1, world), 1 << 20, np.int32)
                cnt0 = mc.canary((world + 8,), 1 << 20, np.int32)
                record, dest, bc, cnt = _dev(record0), _dev(dest0), _dev(bc0), _dev(cnt0)
                assert lib.cgnn_rollout_advance(
                    hist.data_ptr(), w, p["cap"], n, phase, ids.data_ptr(), _ptr(pred_row), _inner(acc).data_ptr(),
                    _inner(rate).data_ptr(), n, stats, mc.DT, box, grid[0], grid[1], grid[2], int(tiles == "planes"),
                    _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), record.data_ptr(), dest.data_ptr(), bc.data_ptr(),
                    cnt.data_ptr(), _stream()) == 0, what
                record0[:n], dest0[:n] = p["want_record"], p["want_dest"]
                bc0[:-1] = mc.block_counts(p["want_mask"], world)
                cnt0[:world] = mc.counts(p["want_mask"], world)
                mc.assert_bits(record, record0, what + " record")
                mc.assert_bits(hist, p["want_hist"], what + " ring")
                mc.assert_bits(dest, dest0, what + " dest")
                mc.assert_bits(bc, bc0, what + " block_counts")
                mc.assert_bits(cnt, cnt0, what + " counts")
    p = mc.advance_problem(world, 257, w, 1, grid, 1.0, tiles == "planes", True)       # the wrapper: the same bits
    meta = dict(dt=mc.DT, box_size=1.0)
    hist = _dev(p["hist"])
    record, dest, bc, cnt = ops.rollout_advance(hist, 257, 1, _dev(p["ids"]), _dev(p["acc"]), _dev(p["rate"]), meta, grid,
                                                None if p["planes"] is None else [_dev(c) for c in p["planes"]],
                                                pred_row=_dev(p["pred_row"]), stats=stats)
    mc.assert_bits(record, p["want_record"], "ops.rollout_advance record")
    mc.assert_bits(hist, p["want_hist"], "ops.rollout_advance ring")
    mc.assert_bits(dest, p["want_dest"], "ops.rollout_advance dest")
    mc.assert_bits(bc, mc.block_counts(p["want_mask"], world), "ops.rollout_advance block_counts")


# ---- cgnn_migrate_pack / cgnn_migrate_unpack --------------------------------------------------------------------------------
def _pack(lib, c):
    hist, ids, dest = _dev(c["hist"]), _dev(c["ids"]), _dev(mc.padded(c["dest"], -1))
    offsets = ops.group_offsets(_dev(mc.block_counts(c["mask"], c["world"])), _dev(c["starts"]))
    hist_out, ids_out, send = _dev(c["hist_out0"]), _dev(c["ids_out0"]), _dev(c["send0"])
    rc = lib.cgnn_migrate_pack(hist.data_ptr(), c["w"], c["cap"], c["n"], ids.data_ptr(), _inner(dest).data_ptr(), c["world"],
                               c["rank"], offsets.data_ptr(), _ptr(hist_out), c["cap_out"], _ptr(ids_out), send.data_ptr(),
                               c["n_send"], _stream())
    return rc, hist_out, ids_out, send


@pytest.mark.parametrize("w", mc.MIGRATE_WINDOWS)
@pytest.mark.parametrize("world", mc.MIGRATE_WORLDS)
@pytest.mark.parametrize("name", mc.DEST_PATTERNS)
def test_migrate_pack_and_unpack_move_every_history_to_its_place(name, world, w):
    """Every destination pattern at every size of N_EDGES, rank 0 and world - 1: the second ring, ids_out and the send buffer
    equal the reference everywhere, canaries included; with cap_out below the stayers and n_send below the leavers (both
    guards), with starts 2 lower (``at < 0``), and with invalid destinations, which take no place.  Then every peer's block of
    the send buffer is unpacked behind ``first`` stayers of a fresh ring, with first + R == cap_out."""
    lib = _lib.load()
    for n in mc.N_EDGES:
        for rank in sorted({0, world - 1}):
            for layout in mc.START_LAYOUTS:
                c = mc.migrate_pack_case(name, n, world, rank, w, layout)
                what = f"migrate_pack {name} world {world} rank {rank} W {w} n {n} {layout}"
                rc, hist_out, ids_out, send = _pack(lib, c)
                assert rc == 0, what
                mc.assert_bits(hist_out, c["want_hist_out"], what + " second ring")
                mc.assert_bits(ids_out, c["want_ids_out"], what + " ids_out")
                mc.assert_bits(send, c["want_send"], what + " send")
                if layout != "packed":
                    continue
                cnt = mc.counts(c["mask"], world)
                for peer in sorted({p for p in (0, 1, world - 2, world - 1) if 0 <= p < world and p != rank and cnt[p]}):
                    r, first = int(cnt[peer]), 4 + peer % 3
                    block = send[int(c["starts"][peer]):int(c["starts"][peer]) + r]
                    ring0, ring_ids0 = mc.canary((w, first + r, 4), 5000.0), mc.canary((first + r,), 1 << 21, np.int32)
                    ring, ring_ids = _dev(ring0), _dev(ring_ids0)
                    assert lib.cgnn_migrate_unpack(block.data_ptr(), r, w, ring.data_ptr(), first + r, first,
                                                   ring_ids.data_ptr(), _stream()) == 0
                    want_ring, want_ids = mc.migrate_unpack_ref(c["want_send"][int(c["starts"][peer]):][:r], ring0, ring_ids0,
                                                                first)
                    mc.assert_bits(ring, want_ring, what + f" unpack of peer {peer}")
                    mc.assert_bits(ring_ids, want_ids, what + f" unpacked ids of peer {peer}")
                    rows = np.nonzero(c["dest"] == peer)[0]
                    mc.assert_bits(want_ring[:, first:], c["hist"][:, rows], what + " the leavers' histories")
                    assert want_ids[first:].tolist() == c["ids"][rows].tolist()


def test_a_world_of_eight_packs_and_unpacks_every_id_exactly_once():
    """Round trip through the wrappers: every rank packs its rows (a different number on every rank, wave and block edges
    among them), the blocks are dealt as dist.exchange_rows deals them, every rank unpacks behind its stayers."""
    world, w = 8, 5
    held = (1, 63, 64, 65, 255, 256, 257, 1025)
    gen = np.random.default_rng(8)
    ranks, next_id = [], 0
    for rank, n in enumerate(held):
        hist, _ = mc.ring(gen, w, n, n + 9, 1.0)
        ids = np.full(n + 9, -5, dtype=np.int32)
        ids[:n] = next_id + gen.permutation(n)
        next_id += n
        dest = gen.integers(0, world, size=n).astype(np.int32)
        dest[n // 2:] = rank if rank % 2 else dest[n // 2:]
        ranks.append(dict(hist=hist, ids=ids, dest=dest, n=n, cnt=mc.counts(mc.dest_mask(dest, world), world)))
    arriving = [sum(int(r["cnt"][me]) for k, r in enumerate(ranks) if k != me) for me in range(world)]
    sends, send_counts, rings = [], [], []
    for rank, r in enumerate(ranks):
        starts, _, n_send = mc.migrate_layout("packed", r["cnt"], rank)
        cap_out = int(r["cnt"][rank]) + arriving[rank]
        ring, ring_ids = _dev(mc.canary((w, cap_out, 4), 5000.0)), _dev(mc.canary((cap_out,), 1 << 21, np.int32))
        offsets = ops.group_offsets(_dev(mc.block_counts(mc.dest_mask(r["dest"], world), world)), _dev(starts))
        send = ops.migrate_pack(_dev(r["hist"]), r["n"], _dev(r["ids"]), _dev(r["dest"]), rank, offsets, ring, ring_ids, n_send)
        sends.append(send.cpu().numpy())
        send_counts.append([0 if p == rank else int(c) for p, c in enumerate(r["cnt"])])
        rings.append((ring, ring_ids))
    want = {}
    for r in ranks:
        for i in range(r["n"]):
            want[int(r["ids"][i])] = (int(r["dest"][i]), r["hist"][:, i])
    seen = set()
    for me, (ring, ring_ids) in enumerate(rings):
        arrivals = mc.split_arrivals(sends, send_counts, me)
        assert arrivals.shape[0] == arriving[me]
        ops.migrate_unpack(_dev(arrivals), ring, ring_ids, int(ranks[me]["cnt"][me]))
        got_ring, got_ids = ring.cpu().numpy(), ring_ids.cpu().numpy()
        for row, gid in enumerate(got_ids.tolist()):
            assert gid in want and gid not in seen and want[gid][0] == me, (me, row, gid)
            seen.add(gid)
            mc.assert_bits(got_ring[:, row], want[gid][1], f"id {gid} on rank {me}")
    assert seen == set(want) and len(seen) == sum(held)


# ---- cgnn_history_features --------------------------------------------------------------------------------------------------
def _features(lib, p, rows, what):
    """One call with canaries in and behind x and recent -> nothing; asserts the bits of features_ref."""
    w, n_held = p["w"], p["n_held"]
    nr = n_held if rows is None else len(rows)
    x0, recent0 = mc.canary((nr + PAD_ROWS, 4 * w - 3)), mc.canary((nr + PAD_ROWS, 4), 7000.0)
    x, recent = _dev(x0), _dev(recent0)
    rows_d = None if rows is None else _dev(mc.padded(np.asarray(rows, dtype=np.int32), 0))
    st = p["stats"]
    assert lib.cgnn_history_features(p["hist_d"].data_ptr(), w, p["cap"], n_held, p["phase"],
                                     None if rows is None else _inner(rows_d).data_ptr(), nr, p["ids_d"].data_ptr(), p["box"],
                                     p["dt"], st["vel_mean"], st["vel_std"], st["temp_mean"], st["temp_std"], x.data_ptr(),
                                     recent.data_ptr(), _stream()) == 0, what
    want_x, want_recent = mc.features_ref(p["hist"], p["phase"], rows, n_held, p["ids"], p["box"], p["dt"], st, x0[:nr],
                                          recent0[:nr])
    x0[:nr], recent0[:nr] = want_x, want_recent
    mc.assert_bits(x, x0, what + " x")
    mc.assert_bits(recent, recent0, what + " recent")
    return x


def _feature_problem(seed, w, n_held, phase, box):
    p = mc.features_problem(seed, w, n_held, phase, box)
    p["hist_d"], p["ids_d"] = _dev(p["hist"]), _dev(p["ids"])
    return p


def _row_lists(n_held, cap):
    assert cap - 1 >= n_held
    skipped = np.arange(n_held, dtype=np.int32)[::3].copy()
    skipped[[0, len(skipped) // 2, -1]] = (-1, n_held, cap - 1)
    return dict(reversed=np.arange(n_held, dtype=np.int32)[::-1].copy(), repeated=(np.arange(300, dtype=np.int32) // 3 * 5) % n_held,
                skipped=skipped)


@pytest.mark.parametrize("w", mc.FEATURE_WINDOWS)
def test_history_features_of_every_phase_up_to_the_largest_window(w):
    """W = 16 fills the 64 KiB a kernel gets by default, 17 is the first window that needs the attribute, 32 (128 KiB) the
    documented maximum.  Every phase: all 257 held rows, and row lists that are reversed, repeated, and hold -1, n_held and
    cap - 1 (skipped: those output rows keep their canary in x and in recent).  n_rows 1, 255 and 256 at three phases."""
    lib = _lib.load()
    assert (mc.window_lds_bytes(w) > mc.LDS_DEFAULT) == (w >= mc.FIRST_WINDOW_ABOVE_64K)
    for phase in range(w):
        box = (1.0, 2.0)[phase % 2]
        p = _feature_problem(w + phase, w, 257, phase, box)
        _features(lib, p, None, f"features W {w} phase {phase} all rows")
        for name, rows in _row_lists(p["n_held"], p["cap"]).items():
            _features(lib, p, rows, f"features W {w} phase {phase} {name} rows")
    for phase in sorted({0, w // 2, w - 1}):
        for n in mc.FEATURE_N[:3]:
            _features(lib, _feature_problem(n + phase, w, n, phase, 1.0), None, f"features W {w} phase {phase} n {n}")


def test_the_smallest_window_after_the_largest_gives_the_same_bits():
    """ensure_dynamic_lds keeps the largest size it has set: W = 2 before and after W = 32, then W = 17 under the cached size."""
    lib = _lib.load()
    small, large, mid = (_feature_problem(5, w, 257, 1, 1.0) for w in (2, 32, 17))
    first = _features(lib, small, None, "W 2 first").cpu()
    _features(lib, large, None, "W 32")
    mc.assert_bits(_features(lib, small, None, "W 2 after W 32"), first, "W 2 before and after W 32")
    _features(lib, mid, None, "W 17 after W 32")
    got, _ = ops.history_features(small["hist_d"], 257, 1, small["stats"], mc.DT, 1.0)
    mc.assert_bits(got, first[:257], "ops.history_features")


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_every_entry_refuses_world_65_window_33_and_null_lists_and_writes_nothing():
    lib = _lib.load()
    s = _stream()
    w, cap, n, world = 4, 16, 8, 2
    outputs = dict(hist=mc.canary((w, cap, 4)), spare=mc.canary((w, cap, 4), 2000.0), x=mc.canary((n, 4 * 33 - 3)),
                   recent=mc.canary((n, 4), 3000.0), record=mc.canary((n, mc.ROW)), out=mc.canary((4, 4), 4000.0),
                   send=mc.canary((4, 34, 4), 5000.0), dest=np.zeros(n, dtype=np.int32),
                   bc=mc.canary((1, 65), 1 << 20, np.int32), cnt=mc.canary((65,), 1 << 21, np.int32),
                   mask=mc.canary((n,), 1 << 40, np.int64), ids=np.arange(cap, dtype=np.int32))
    d = {k: _dev(v) for k, v in outputs.items()}
    ptr = {k: v.data_ptr() for k, v in d.items()}
    acc, rate = torch.zeros(n, 3, device=DEV), torch.zeros(n, device=DEV)
    stats = (C.c_float * 8)(*mc.ADVANCE_STATS)
    lo, hi = (C.c_double * (3 * 65))(*([0.0] * 195)), (C.c_double * (3 * 65))(*([1.0] * 195))
    feat = lambda window: lib.cgnn_history_features(ptr["hist"], window, cap, n, 0, None, n, ptr["ids"], 1.0, mc.DT, 0.0,   # noqa: E731
                                                    1.0, 0.0, 1.0, ptr["x"], ptr["recent"], s)
    adv = lambda window, grid, dest: lib.cgnn_rollout_advance(                                                             # noqa: E731
        ptr["hist"], window, cap, n, 1, ptr["ids"], None, acc.data_ptr(), rate.data_ptr(), n, stats, mc.DT, 1.0, *grid, 0,
        None, None, None, ptr["record"], dest, ptr["bc"], ptr["cnt"], s)
    sel = lambda wd, mask: lib.cgnn_halo_select(ptr["recent"], n, wd, 0, lo, hi, 0.1, 1.0, mask, ptr["bc"], ptr["cnt"], s)   # noqa: E731
    hpack = lambda wd, mask, off: lib.cgnn_halo_pack(ptr["recent"], mask, n, wd, off, 4, ptr["out"], s)                    # noqa: E731
    mpack = lambda window, wd, dest, off: lib.cgnn_migrate_pack(ptr["hist"], window, cap, n, ptr["ids"], dest, wd, 0, off,    # noqa: E731
                                                                ptr["spare"], cap, ptr["ids"], ptr["send"], 4, s)
    unpack = lambda window: lib.cgnn_migrate_unpack(ptr["send"], 2, window, ptr["spare"], cap, 0, ptr["ids"], s)           # noqa: E731
    assert feat(33) == INVALID and b"cgnn_history_features" in lib.cgnn_last_error()
    assert adv(33, (2, 1, 1), ptr["dest"]) == INVALID and adv(w, (13, 5, 1), ptr["dest"]) == INVALID
    assert adv(w, (2, 1, 1), None) == INVALID and b"cgnn_rollout_advance" in lib.cgnn_last_error()
    assert sel(65, ptr["mask"]) == INVALID and sel(world, None) == INVALID and b"cgnn_halo_select" in lib.cgnn_last_error()
    assert hpack(65, ptr["mask"], ptr["bc"]) == INVALID and hpack(world, None, ptr["bc"]) == INVALID
    assert hpack(world, ptr["mask"], None) == INVALID and b"cgnn_halo_pack" in lib.cgnn_last_error()
    assert mpack(33, world, ptr["dest"], ptr["bc"]) == INVALID and mpack(w, 65, ptr["dest"], ptr["bc"]) == INVALID
    assert mpack(w, world, None, ptr["bc"]) == INVALID and mpack(w, world, ptr["dest"], None) == INVALID
    assert b"cgnn_migrate_pack" in lib.cgnn_last_error()
    assert unpack(33) == INVALID and b"cgnn_migrate_unpack" in lib.cgnn_last_error()
    torch.cuda.synchronize()
    for k, before in outputs.items():
        mc.assert_bits(d[k], before, f"{k} after the refused calls")
